// half_bits.h -- binary32 -> binary16 conversion of the scene's normals, shared by scene creation (scene_create.hip) and the refit
// (refit/refit.hip) so that both produce the same fp16 normals bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

namespace {

// binary32 -> binary16 bits, round to nearest even (GL_RGB16F upload, ray.cpp:474)
__host__ __device__ uint16_t float_to_half_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    uint32_t mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u)
        return sign | 0x7e00u;                      // NaN
    if (mag >= 0x477ff000u)
        return sign | 0x7c00u;                      // overflow -> inf (also inf itself)
    if (mag < 0x33000001u)
        return sign;                                // rounds to zero (<= 2^-25)
    if (mag < 0x38800000u) {                        // subnormal half
        const int shift = 126 - (int)(mag >> 23);   // 14..24
        const uint32_t mant = (mag & 0x7fffffu) | 0x800000u;
        const uint32_t q = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1u);
        const uint32_t halfway = 1u << (shift - 1);
        const uint32_t up = (rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u;
        return sign | (uint16_t)(q + up);
    }
    const uint32_t lsb = (mag >> 13) & 1u;
    mag += 0xfffu + lsb;
    return sign | (uint16_t)((mag - 0x38000000u) >> 13);
}

}   // namespace
