// triangle_box_test.h -- the per-triangle arithmetic of include/shader_ray_overlap.h, shared by the box-overlap walk
// (overlap/overlap.hip) and its instanced form (instance_overlap/instance_overlap.hip), so that both compile the same code and
// a box's set is the same wherever it is computed: the header's min and max, its 13-axis triangle/box test, and the cull of
// a node's box against a query box.  The triangle-intersection walks (triangle_pair_test.h) take the min and max and the
// cull from here.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "packed_walk.h"

namespace {

// the header's min and max: comparisons, so that a NaN is passed on or dropped as the header's are
__device__ __forceinline__ float min2(float x, float y) { return x < y ? x : y; }
__device__ __forceinline__ float max2(float x, float y) { return x > y ? x : y; }
__device__ __forceinline__ float min3(float x, float y, float z) { return min2(min2(x, y), z); }
__device__ __forceinline__ float max3(float x, float y, float z) { return max2(max2(x, y), z); }

// one edge axis of stage 2: the corners' projections p0, p1, p2 against the box's radius r
__device__ __forceinline__ bool separated(float p0, float p1, float p2, float r)
{
    return min3(p0, p1, p2) > r || max3(p0, p1, p2) < -r;
}

// the three axes (edge x box axis) of one edge e over the corners v0, v1, v2
__device__ __forceinline__ bool edge_separates(const float e[3], const float v0[3], const float v1[3], const float v2[3], const float h[3])
{
    const float ax = fabsf(e[0]), ay = fabsf(e[1]), az = fabsf(e[2]);
    if (separated(e[1] * v0[2] - e[2] * v0[1], e[1] * v1[2] - e[2] * v1[1], e[1] * v2[2] - e[2] * v2[1], h[1] * az + h[2] * ay))
        return true;
    if (separated(e[2] * v0[0] - e[0] * v0[2], e[2] * v1[0] - e[0] * v1[2], e[2] * v2[0] - e[0] * v2[2], h[0] * az + h[2] * ax))
        return true;
    return separated(e[0] * v0[1] - e[1] * v0[0], e[0] * v1[1] - e[1] * v1[0], e[0] * v2[1] - e[1] * v2[0], h[0] * ay + h[1] * ax);
}

// the header's per-triangle test: the box (lo, hi), its centre m and half extent h, the triangle's nine floats
__device__ __forceinline__ bool triangle_overlaps(const float lo[3], const float hi[3], const float m[3], const float h[3], const float *tri)
{
    float a[3], b[3], c[3];
#pragma unroll
    for (int j = 0; j < 3; j++)
        a[j] = tri[j], b[j] = tri[3 + j], c[j] = tri[6 + j];
    // stage 0: the box's axes, on the untranslated coordinates
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (min3(a[j], b[j], c[j]) > hi[j] || max3(a[j], b[j], c[j]) < lo[j])
            return false;
    float v0[3], v1[3], v2[3], e0[3], e1[3], e2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        v0[j] = a[j] - m[j], v1[j] = b[j] - m[j], v2[j] = c[j] - m[j];
        e0[j] = v1[j] - v0[j], e1[j] = v2[j] - v1[j], e2[j] = v0[j] - v2[j];
    }
    // stage 1: the triangle's plane
    const float nx = e0[1] * e1[2] - e0[2] * e1[1], ny = e0[2] * e1[0] - e0[0] * e1[2], nz = e0[0] * e1[1] - e0[1] * e1[0];
    const float d = (nx * v0[0] + ny * v0[1]) + nz * v0[2];
    const float r = (h[0] * fabsf(nx) + h[1] * fabsf(ny)) + h[2] * fabsf(nz);
    if (d > r || d < -r)
        return false;
    // stage 2: edge x box axis
    return !(edge_separates(e0, v0, v1, v2, h) || edge_separates(e1, v0, v1, v2, h) || edge_separates(e2, v0, v1, v2, h));
}

// a walk's cull: the node's box against the query box (a query triangle's vertex box), six comparisons of stored floats
__device__ __forceinline__ bool boxes_overlap(const Box &node, const float lo[3], const float hi[3])
{
    return !(node.hi[0] < lo[0] || node.lo[0] > hi[0] || node.hi[1] < lo[1] || node.lo[1] > hi[1] || node.hi[2] < lo[2] ||
             node.lo[2] > hi[2]);
}

}   // namespace
