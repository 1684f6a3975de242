// winding_walk.h -- the winding number's walk (include/shader_ray_winding.h): a far node's term, a
// triangle's exact term, and the depth-first walk over a scene's node records and octant copy 7 of its packed tree.
// winding/winding.hip runs it on a scene; instance_winding/instance_winding.hip runs it on each member of a set in object
// space.  Device code only, compiled by each library that includes it; no kernel here.
#pragma once

#include <hip/hip_runtime.h>

#include "packed_walk.h"
#include "trace_common.h"

namespace {

using namespace shray;

constexpr float kInv4Pi = (float)(1.0 / (4.0 * 3.14159265358979323846));
constexpr float kInv2Pi = (float)(1.0 / (2.0 * 3.14159265358979323846));

__device__ __forceinline__ V3 corner(const float *c9, int j) { return mk(c9[3 * j], c9[3 * j + 1], c9[3 * j + 2]); }

// the far-field term of a node whose { P, r } gave d and d2
__device__ __forceinline__ float far_term(const float4 *__restrict__ rec, V3 d, float d2)
{
    const float4 w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4];
    const float len = sqrtf(d2);
    const float i3 = 1.0f / (d2 * len);
    const float i5 = i3 / d2;
    const float tr = (w2.x + w3.x) + w4.x;   // M_00 + M_11 + M_22
    const V3 m = mk((w2.x * d.x + w2.y * d.y) + w2.z * d.z, (w2.w * d.x + w3.x * d.y) + w3.y * d.z, (w3.z * d.x + w3.w * d.y) + w4.x * d.z);
    return (((dot3(mk(w1.x, w1.y, w1.z), d) + tr) * i3) - ((3.0f * dot3(d, m)) * i5)) * kInv4Pi;
}

// the exact term of triangle t (its signed solid angle over 4 pi)
__device__ __forceinline__ float triangle_term(const float *c9, V3 q)
{
    const V3 a = corner(c9, 0) - q, b = corner(c9, 1) - q, c = corner(c9, 2) - q;
    const float det = dot3(a, cross3(b, c));
    const float la = sqrtf(dot3(a, a)), lb = sqrtf(dot3(b, b)), lc = sqrtf(dot3(c, c));
    const float den = (((la * lb) * lc + dot3(a, b) * lc) + dot3(a, c) * lb) + dot3(b, c) * la;
    return det == 0.0f ? 0.0f : atan_yx(det, den) * kInv2Pi;
}

struct WindingView {
    const float4 *records;     // SHRAY_WINDING_DATA_FLOATS floats per node
    const char *copy7;         // octant copy 7 of the packed tree
    const float *positions;
    uint32_t root;             // the root's name
    float beta;
};

// w(q; beta) by the walk of the header; `column` is this lane's stack column in LDS (level-major, kBlock apart)
__device__ __forceinline__ float winding_walk(const WindingView &v, V3 q, uint32_t *column)
{
    float w = 0.0f;
    uint32_t name = v.root;
    int sp = 0;
    while (true) {
        const float4 *rec = v.records + (size_t)5 * (name >> (kNodeShift - kNodeNameShift));
        const float4 pr = rec[0];
        const V3 d = mk(pr.x - q.x, pr.y - q.y, pr.z - q.z);
        const float d2 = dot3(d, d);
        const float br = v.beta * pr.w;
        if (d2 > br * br) {
            w = w + far_term(rec, d, d2);
        } else {
            const uint2 ab = *reinterpret_cast<const uint2 *>(v.copy7 + ((size_t)name << kNodeNameShift) + 24);
            if (!(ab.y & kLeafFlag)) {
                column[(size_t)sp * kBlock] = ab.y;   // the positive child, after the negative subtree
                sp++;
                name = ab.x & kChildNameMask;
                continue;
            }
            const uint32_t end = ab.x + (ab.y & ~kLeafFlag);
            for (uint32_t t = ab.x; t < end; t++)
                w = w + triangle_term(v.positions + 9ull * t, q);
        }
        if (sp == 0)
            break;
        sp--;
        name = column[(size_t)sp * kBlock];
    }
    return w;
}

}   // namespace
