// image_box.h -- the geometry that the instanced walks over a member's packed tree share (instance_point/, instance_near/,
// instance_overlap/, instance_intersect/), so that all compile the same code: a node's box and a triangle's corners under an
// instance's forward map, the culls on an image box, and the guarded cull of a top-level node's stored box.  Like
// enter_set.h it needs point/'s headers (Box of packed_walk.h, box_bound of closest_on_triangle.h), which
// libshray_instance.so's own units, built without -Ipoint, do not see: they must not include it.  Internal to the libraries;
// no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "closest_on_triangle.h"
#include "packed_walk.h"
#include "trace_common.h"

namespace {

// the image of a node's box under the map's rows: per world axis the corner formula on the ends that make it smallest and
// largest, chosen by the signs of the row's entries alone (a zero entry is not read: either end)
__device__ __forceinline__ Box image_box(const float4 (&m)[3], const Box &b)
{
    Box o;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float row[3] = {m[r].x, m[r].y, m[r].z};
        float lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = row[c] < 0.0f ? b.hi[c] : b.lo[c];
            hi[c] = row[c] < 0.0f ? b.lo[c] : b.hi[c];
        }
        o.lo[r] = object_row(m[r], mk(lo[0], lo[1], lo[2]), true);
        o.hi[r] = object_row(m[r], mk(hi[0], hi[1], hi[2]), true);
    }
    return o;
}

// a member node's cull by distance: the box bound of its image box from the point p
__device__ __forceinline__ float image_bound(const float4 (&m)[3], const float p[3], const Box &b)
{
    const Box o = image_box(m, b);
    return box_bound(p, o.lo, o.hi);
}

// a member node's cull by overlap: its image box against the query box (a query triangle's vertex box), six comparisons; a
// NaN end compares false and culls less
__device__ __forceinline__ bool image_overlaps(const float4 (&m)[3], const Box &node, const float lo[3], const float hi[3])
{
    const Box o = image_box(m, node);
    return !(o.hi[0] < lo[0] || o.lo[0] > hi[0] || o.hi[1] < lo[1] || o.lo[1] > hi[1] || o.hi[2] < lo[2] || o.lo[2] > hi[2]);
}

// use(c9) on triangle t of `positions` under the map m: nine world floats (include/shader_ray_instance_point.h's formula).
// The corners are handed to a callable, not written through a pointer, so that the array is this function's own: that is
// the form whose instructions are the ones each walk had when it spelled the loop out.
template <class Use>
__device__ __forceinline__ auto with_mapped_corners(const float4 (&m)[3], const float *positions, uint64_t t, Use &&use)
{
    const float *v = positions + 9ull * t;
    float c9[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V3 corner = mk(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
#pragma unroll
        for (int r = 0; r < 3; r++)
            c9[3 * k + r] = object_row(m[r], corner, true);
    }
    return use(c9);
}

// the same nine floats into the caller's array
__device__ __forceinline__ void mapped_corners(const float4 (&m)[3], const float *positions, uint64_t t, float out[9])
{
    with_mapped_corners(m, positions, t, [&](const float *c9) {
#pragma unroll
        for (int i = 0; i < 9; i++)
            out[i] = c9[i];
    });
}

// Below this magnitude a stored top-level float and the query float beside it may not separate an axis.  place_box's margin,
// 128 u s (|Y| + |b|), covers the three half subnormal steps by which an fp32 corner can leave its exact image as soon as the
// box's largest coordinate reaches 2^-109 (DESIGN sections 20 and 23), so a corner outside its stored box, the stored end it
// passed and any query end between the two are all below 2^-109.
constexpr float kGuard = 0x1p-109f;

// one comparison of a top-level node's cull: the stored end lies beyond the query end, and the two are not both near zero
__device__ __forceinline__ bool guarded(bool beyond, float stored, float query)
{
    return beyond && !(fabsf(stored) < kGuard && fabsf(query) < kGuard);
}

// a top-level node's cull: its stored box (a, b) against the query box (a query triangle's vertex box)
__device__ __forceinline__ bool stored_overlaps(const float4 &a, const float4 &b, const float lo[3], const float hi[3])
{
    return !(guarded(b.x < lo[0], b.x, lo[0]) || guarded(a.x > hi[0], a.x, hi[0]) || guarded(b.y < lo[1], b.y, lo[1]) ||
             guarded(a.y > hi[1], a.y, hi[1]) || guarded(b.z < lo[2], b.z, lo[2]) || guarded(a.z > hi[2], a.z, hi[2]));
}

}   // namespace
