// point_walk.h -- the closest-point walk of include/shader_ray_point.h, shared by libshray_point.so (point/point.hip) and
// libshray_sdf.so (sdf/sdf.hip), so that both compile the same code and a signed-distance record's closest part is the
// closest-point record bit for bit.
//
// One lane per point walks the packed tree (packed_layout.h) with a stack in LDS, nearest child first.  The boxes come from
// octant copy 7, whose entry / exit planes are boxmin / boxmax; the corners from the scene's positions.  A node is skipped
// only when its box bound is strictly above the best dist2 so far, which makes the walk's answer the brute-force answer of
// the header, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "client_internal.h"
#include "device_types.h"
#include "error_internal.h"
#include "packed_layout.h"
#include "packed_walk.h"
#include "scene_access_internal.h"
#include "shader_ray_point.h"

namespace {

using namespace shray;


constexpr uint64_t kPointsPerLaunch = 1ull << 24;   // the grid's threads stay far below 2^32

// the stack of one workgroup: (node name, box bound) per level, level-major so that a wave's accesses are consecutive
inline size_t stack_bytes(int height) { return (size_t)kBlock * (size_t)(height > 0 ? height : 1) * sizeof(uint2); }

struct PointWork {
    const float4 *points;   // (p, max_dist2)
    float4 *out;            // 2 per point: (q, dist2), (u, v, triangle bits, region bits)
    uint64_t count;
    uint64_t first;         // this launch's first point
    DeviceCounters *counters;
};

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

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x += __shfl_xor(x, off);
    return x;
}

// One lane per point.  COUNT: the counting instance (node_visits, leaf_visits, triangle_tests into kCounterShards shards).
template <bool COUNT>
__global__ void __launch_bounds__(kBlock) closest_point_kernel(SceneView sc, PointWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint2 stack[];
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 in = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (live)
        in = w.points[index];
    const float p[3] = {in.x, in.y, in.z};
    const bool walk = live && __builtin_isfinite(in.x) && __builtin_isfinite(in.y) && __builtin_isfinite(in.z) && in.w >= 0.0f;

    float best = in.w;   // the best dist2, max_dist2 until a triangle qualifies
    int best_tri = SHRAY_HIT_MISS;
    Closest found;
    found.q[0] = p[0], found.q[1] = p[1], found.q[2] = p[2];
    found.u = 0.0f, found.v = 0.0f, found.region = SHRAY_REGION_NONE;
    unsigned int nodes = 0, leaves = 0, tests = 0;

    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    uint2 *column = stack + threadIdx.x;
    if (walk) {
        Record cur = load_record(copy, sc.packed_root);
        nodes++;
        int sp = 0;
        bool go = !(box_bound(p, cur.box.lo, cur.box.hi) > best);
        while (go) {
            if (cur.b & kLeafFlag) {
                leaves++;
                const uint32_t first = cur.a, n = cur.b & ~kLeafFlag;
                for (uint32_t t = first; t < first + n; t++) {
                    tests++;
                    const Closest c = closest_on_triangle(p, sc.positions + 9ull * t);
                    const bool better = best_tri < 0 ? c.dist2 <= best : (c.dist2 < best || (c.dist2 == best && (int)t < best_tri));
                    if (better) {
                        best = c.dist2;
                        best_tri = (int)t;
                        found = c;
                    }
                }
            } else {
                const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
                const float lb0 = box_bound(p, r0.box.lo, r0.box.hi), lb1 = box_bound(p, r1.box.lo, r1.box.hi);
                nodes += 2;
                const bool second = lb1 < lb0;   // the nearer child first
                const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
                if (!(near_lb > best)) {
                    if (!(far_lb > best)) {
                        column[(size_t)sp * kBlock] = make_uint2(second ? n0 : n1, __float_as_uint(far_lb));
                        sp++;
                    }
                    cur = second ? r1 : r0;
                    continue;
                }
                // near_lb <= far_lb: both children are out of reach
            }
            // pop the next node still in reach; the stack holds at most one entry per level of the current path
            go = false;
            while (sp > 0) {
                sp--;
                const uint2 e = column[(size_t)sp * kBlock];
                if (!(__uint_as_float(e.y) > best)) {
                    cur = load_record(copy, e.x);
                    go = true;
                    break;
                }
            }
        }
    }
    if (live) {
        const bool hit = best_tri >= 0;
        w.out[2 * index] = make_float4(found.q[0], found.q[1], found.q[2], hit ? best : in.w);
        w.out[2 * index + 1] = make_float4(found.u, found.v, __int_as_float(best_tri), __int_as_float(found.region));
    }
    if (COUNT) {
        const unsigned long long s0 = wave_sum(nodes), s1 = wave_sum(leaves), s2 = wave_sum(tests);
        if (threadIdx.x == 0) {
            DeviceCounters *c = &w.counters[blockIdx.x % kCounterShards];
            atomicAdd(&c->node_visits, s0);
            atomicAdd(&c->leaf_visits, s1);
            atomicAdd(&c->triangle_tests, s2);
        }
    }
}

// `count` > 0 points -> records on `stream`, split over launches (the arguments are checked, the scene is walkable)
inline int enqueue_closest(const ShrayQueryScene &q, int height, const shray_point *d_points, uint64_t count, shray_closest *d_out,
                           hipStream_t stream, DeviceCounters *d_counters)
{
    PointWork w{(const float4 *)d_points, (float4 *)d_out, count, 0, d_counters};
    const size_t lds = stack_bytes(height);
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    return for_each_launch(blocks, kPointsPerLaunch / kBlock, [&](uint64_t first, dim3 grid) {
        w.first = first * kBlock;
        if (d_counters)
            hipLaunchKernelGGL(closest_point_kernel<true>, grid, dim3(kBlock), lds, stream, q.view, w);
        else
            hipLaunchKernelGGL(closest_point_kernel<false>, grid, dim3(kBlock), lds, stream, q.view, w);
        return launched("closest-point");
    });
}

}   // namespace
