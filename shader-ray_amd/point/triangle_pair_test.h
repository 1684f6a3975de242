// triangle_pair_test.h -- the per-pair arithmetic of include/shader_ray_intersect.h, shared by the triangle-intersection walk
// (intersect/intersect.hip) and its instanced form (instance_intersect/instance_intersect.hip), so that both compile the same
// code and a query's set is the same wherever it is computed: what a lane keeps of its query triangle, and the header's
// 17-axis triangle/triangle test, over triangle_box_test.h's min and max.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "triangle_box_test.h"

namespace {

__device__ __forceinline__ float dot(const float x[3], const float y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ __forceinline__ void cross(float out[3], const float x[3], const float y[3])
{
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

__device__ __forceinline__ bool all_zero(const float x[3]) { return x[0] == 0.0f && x[1] == 0.0f && x[2] == 0.0f; }

__device__ __forceinline__ bool same_corner(const float x[3], const float y[3]) { return x[0] == y[0] && x[1] == y[1] && x[2] == y[2]; }

// What a lane keeps of its query: the corners (stage 0's box is lo, hi; the shared-corner stage compares p), the translated
// corners q1 and q2 (q0 is exactly 0 for the finite queries that are walked) and the normal.  The edges (f0 = q1 - q0,
// f1 = q2 - q1, f2 = q0 - q2) and the in-plane axes nq x f are recomputed per pair, after the stages that reject most.
struct Query {
    float p[3][3];
    float lo[3], hi[3];
    float q1[3], q2[3];
    float nq[3];
};

// the query's interval on axis A: q0 = 0 is projected like the others (an infinite A gives the header's NaN)
__device__ __forceinline__ bool axis_separates(const float A[3], const float v0[3], const float v1[3], const float v2[3], const Query &q)
{
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float s0 = dot(A, v0), s1 = dot(A, v1), s2 = dot(A, v2);
    const float t0 = dot(A, zero), t1 = dot(A, q.q1), t2 = dot(A, q.q2);
    return min3(s0, s1, s2) > max3(t0, t1, t2) || max3(s0, s1, s2) < min3(t0, t1, t2);
}

// the header's per-pair test of the triangle at `tri` (nine floats, in the query's space)
__device__ __forceinline__ bool triangle_intersects(const Query &q, bool skip_shared, const float *tri)
{
    float a[3], b[3], c[3];
#pragma unroll
    for (int j = 0; j < 3; j++)
        a[j] = tri[j], b[j] = tri[3 + j], c[j] = tri[6 + j];
    // stage 0: the two vertex boxes, on the untranslated coordinates
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (min3(a[j], b[j], c[j]) > q.hi[j] || max3(a[j], b[j], c[j]) < q.lo[j])
            return false;
    if (skip_shared) {
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (same_corner(a, q.p[i]) || same_corner(b, q.p[i]) || same_corner(c, q.p[i]))
                return false;
    }
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float v[3][3], e[3][3], f[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        v[0][j] = a[j] - q.p[0][j], v[1][j] = b[j] - q.p[0][j], v[2][j] = c[j] - q.p[0][j];
        e[0][j] = v[1][j] - v[0][j], e[1][j] = v[2][j] - v[1][j], e[2][j] = v[0][j] - v[2][j];
        f[0][j] = q.q1[j] - zero[j], f[1][j] = q.q2[j] - q.q1[j], f[2][j] = zero[j] - q.q2[j];
    }
    float nt[3];
    cross(nt, e[0], e[1]);
    if (all_zero(nt))
        return false;
    if (axis_separates(q.nq, v[0], v[1], v[2], q) || axis_separates(nt, v[0], v[1], v[2], q))
        return false;
    float A[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            cross(A, f[i], e[j]);
            if (axis_separates(A, v[0], v[1], v[2], q))
                return false;
        }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        cross(A, q.nq, f[i]);
        if (axis_separates(A, v[0], v[1], v[2], q))
            return false;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        cross(A, nt, e[j]);
        if (axis_separates(A, v[0], v[1], v[2], q))
            return false;
    }
    return true;
}

}   // namespace
