// triangle_pair_distance.h -- the per-pair arithmetic of include/shader_ray_clearance.h, shared so that a later instanced form
// compiles the same code and a record is the same bits wherever it is computed: the header's fifteen features (corner against
// triangle both ways through closest_on_triangle.h's closest_on_triangle, edge against edge by Ericson 5.1.9 with zero
// thresholds) taken one after another against a running minimum, the intersecting stage through triangle_pair_test.h's
// 17-axis test, and the box-to-box bound of the walk.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "closest_on_triangle.h"
#include "shader_ray_clearance.h"
#include "triangle_pair_test.h"

namespace {

__device__ __forceinline__ float clamp01(float s)
{
    s = finite_or_zero(s);
    return s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
}

// the header's bound: the squared gap between the query's vertex box (qlo, qhi) and a box (lo, hi), per axis 0 where they meet
__device__ __forceinline__ float box_gap2(const float qlo[3], const float qhi[3], const float lo[3], const float hi[3])
{
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        g[k] = qlo[k] > hi[k] ? qlo[k] - hi[k] : (lo[k] > qhi[k] ? lo[k] - qhi[k] : 0.0f);
    return dot(g, g);
}

// What a lane keeps of its query from its nine floats, as intersect/intersect.hip builds it; returns whether every
// coordinate is finite.
__device__ __forceinline__ bool make_query(Query &q)
{
    bool finite = true;
    float f0[3], f1[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        finite = finite && __builtin_isfinite(q.p[0][j]) && __builtin_isfinite(q.p[1][j]) && __builtin_isfinite(q.p[2][j]);
        q.lo[j] = min3(q.p[0][j], q.p[1][j], q.p[2][j]);
        q.hi[j] = max3(q.p[0][j], q.p[1][j], q.p[2][j]);
        const float q0 = q.p[0][j] - q.p[0][j];
        q.q1[j] = q.p[1][j] - q.p[0][j];
        q.q2[j] = q.p[2][j] - q.p[0][j];
        f0[j] = q.q1[j] - q0;
        f1[j] = q.q2[j] - q.q1[j];
    }
    cross(q.nq, f0, f1);
    return finite;
}

struct PairDistance {
    float x[3], y[3], dist2;   // the witnesses on the query and on the scene triangle
    int feature;
};

// one edge feature: the segment (P, Qe) of the query against the segment (R, S) of the scene triangle
__device__ __forceinline__ void edge_edge(const float P[3], const float Qe[3], const float R[3], const float S[3], int feature, PairDistance &best)
{
    float d1[3], d2[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d1[k] = Qe[k] - P[k];
        d2[k] = S[k] - R[k];
        r[k] = P[k] - R[k];
    }
    const float A = dot(d1, d1), E = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
    float s = 0.0f, t = 0.0f;
    if (!(A > 0.0f) && !(E > 0.0f)) {
        // both are points
    } else if (!(A > 0.0f)) {
        t = clamp01(f / E);
    } else if (!(E > 0.0f)) {
        s = clamp01((-c) / A);
    } else {
        const float den = A * E - b * b;
        s = den != 0.0f ? clamp01((b * f - c * E) / den) : 0.0f;
        t = finite_or_zero((b * s + f) / E);
        if (t < 0.0f) {
            t = 0.0f;
            s = clamp01((-c) / A);
        } else if (t > 1.0f) {
            t = 1.0f;
            s = clamp01((b - c) / A);
        }
    }
    float x[3], y[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        x[k] = pick_min(pick_max(P[k] + d1[k] * s, pick_min(P[k], Qe[k])), pick_max(P[k], Qe[k]));
        y[k] = pick_min(pick_max(R[k] + d2[k] * t, pick_min(R[k], S[k])), pick_max(R[k], S[k]));
        d[k] = x[k] - y[k];
    }
    const float dist2 = dot(d, d);
    if (dist2 < best.dist2) {
        best.dist2 = dist2;
        best.feature = feature;
#pragma unroll
        for (int k = 0; k < 3; k++)
            best.x[k] = x[k], best.y[k] = y[k];
    }
}

// the header's (dist2, feature, x, y) of the query against the triangle at `tri` (nine floats)
__device__ __forceinline__ PairDistance pair_distance(const Query &q, const float *tri)
{
    float v[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            v[i][j] = tri[3 * i + j];
    PairDistance best;
    // features 0-2: the query's corners against the triangle
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const Closest c = closest_on_triangle(q.p[i], tri);
        if (i == 0 || c.dist2 < best.dist2) {
            best.dist2 = c.dist2;
            best.feature = i;
#pragma unroll
            for (int k = 0; k < 3; k++)
                best.x[k] = q.p[i][k], best.y[k] = c.q[k];
        }
    }
    // features 3-5: the triangle's corners against the query
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const Closest c = closest_on_triangle(v[i], &q.p[0][0]);
        if (c.dist2 < best.dist2) {
            best.dist2 = c.dist2;
            best.feature = 3 + i;
#pragma unroll
            for (int k = 0; k < 3; k++)
                best.x[k] = c.q[k], best.y[k] = v[i][k];
        }
    }
    // features 6-14: edge against edge
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            edge_edge(q.p[i], q.p[(i + 1) % 3], v[j], v[(j + 1) % 3], 6 + 3 * i + j, best);
    // the intersecting stage: the witnesses stay
    if (!all_zero(q.nq) && triangle_intersects(q, false, tri)) {
        best.dist2 = 0.0f;
        best.feature = SHRAY_PAIR_INTERSECTING;
    }
    return best;
}

// SHRAY_CLEARANCE_SKIP_SHARED's check: some corner of the triangle at `tri` == some corner of the query
__device__ __forceinline__ bool shares_corner(const Query &q, const float *tri)
{
    bool shared = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            shared = shared || same_corner(tri + 3 * j, q.p[i]);
    return shared;
}

// the bound on the triangle's own vertex box, which may skip a pair before its arithmetic
__device__ __forceinline__ float triangle_gap2(const Query &q, const float *tri)
{
    float lo[3], hi[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        lo[j] = min3(tri[j], tri[3 + j], tri[6 + j]);
        hi[j] = max3(tri[j], tri[3 + j], tri[6 + j]);
    }
    return box_gap2(q.lo, q.hi, lo, hi);
}

}   // namespace
