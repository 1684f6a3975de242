// closest_on_triangle.h -- the per-triangle arithmetic of include/shader_ray_point.h, shared by every library that states an
// answer in its terms (the closest-point walk, point_walk.h, and the within-radius walk, near/near.hip), so that all compile the
// same code and a record is the same bits wherever it is computed: the dot product, the box bound of a node and Ericson's
// closest point on a triangle.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "shader_ray_point.h"

namespace {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ float pick_min(float x, float y) { return x < y ? x : y; }
__device__ __forceinline__ float pick_max(float x, float y) { return x > y ? x : y; }

// the box bound of the header: the squared distance from p to the box, per axis 0 inside the slab
__device__ __forceinline__ float box_bound(const float p[3], const float lo[3], const float hi[3])
{
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        g[k] = p[k] < lo[k] ? lo[k] - p[k] : (p[k] > hi[k] ? p[k] - hi[k] : 0.0f);
    return dot3(g[0], g[1], g[2], g[0], g[1], g[2]);
}

struct Closest {
    float q[3], dist2, u, v;
    int region;
};

__device__ __forceinline__ float finite_or_zero(float s) { return __builtin_isfinite(s) ? s : 0.0f; }

// Ericson's ClosestPtPointTriangle in the header's order of tests, then the clamp to the triangle's vertex box
__device__ __forceinline__ Closest closest_on_triangle(const float p[3], const float *c9)
{
    const float a[3] = {c9[0], c9[1], c9[2]}, b[3] = {c9[3], c9[4], c9[5]}, c[3] = {c9[6], c9[7], c9[8]};
    float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
        bp[k] = p[k] - b[k];
        cp[k] = p[k] - c[k];
    }
    Closest r;
    const float d1 = dot3(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]);
    const float d2 = dot3(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    const float d3 = dot3(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]);
    const float d4 = dot3(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    const float d5 = dot3(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]);
    const float d6 = dot3(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        r.region = SHRAY_REGION_A;
        r.u = 0.0f, r.v = 0.0f;
        for (int k = 0; k < 3; k++)
            r.q[k] = a[k];
    } else if (d3 >= 0.0f && d4 <= d3) {
        r.region = SHRAY_REGION_B;
        r.u = 1.0f, r.v = 0.0f;
        for (int k = 0; k < 3; k++)
            r.q[k] = b[k];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float s = finite_or_zero(d1 / (d1 - d3));
        r.region = SHRAY_REGION_AB;
        r.u = s, r.v = 0.0f;
        for (int k = 0; k < 3; k++)
            r.q[k] = a[k] + ab[k] * s;
    } else if (d6 >= 0.0f && d5 <= d6) {
        r.region = SHRAY_REGION_C;
        r.u = 0.0f, r.v = 1.0f;
        for (int k = 0; k < 3; k++)
            r.q[k] = c[k];
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float s = finite_or_zero(d2 / (d2 - d6));
        r.region = SHRAY_REGION_AC;
        r.u = 0.0f, r.v = s;
        for (int k = 0; k < 3; k++)
            r.q[k] = a[k] + ac[k] * s;
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float s = finite_or_zero((d4 - d3) / ((d4 - d3) + (d5 - d6)));
        r.region = SHRAY_REGION_BC;
        r.u = 1.0f - s, r.v = s;
        for (int k = 0; k < 3; k++)
            r.q[k] = b[k] + (c[k] - b[k]) * s;
    } else {
        const float den = 1.0f / ((va + vb) + vc);
        float u = vb * den, v = vc * den;
        if (!__builtin_isfinite(u) || !__builtin_isfinite(v))
            u = 0.0f, v = 0.0f;
        r.region = SHRAY_REGION_FACE;
        r.u = u, r.v = v;
        for (int k = 0; k < 3; k++)
            r.q[k] = (a[k] + ab[k] * u) + ac[k] * v;
    }
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = pick_min(pick_min(a[k], b[k]), c[k]), hi = pick_max(pick_max(a[k], b[k]), c[k]);
        r.q[k] = pick_min(pick_max(r.q[k], lo), hi);
        d[k] = p[k] - r.q[k];
    }
    r.dist2 = dot3(d[0], d[1], d[2], d[0], d[1], d[2]);
    return r;
}

}   // namespace
