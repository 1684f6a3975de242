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
#include "closest_on_triangle.h"
#include "device_types.h"
#include "error_internal.h"
#include "packed_layout.h"
#include "packed_walk.h"
#include "scene_access_internal.h"
#include "shader_ray_point.h"

namespace {

using namespace shray;

// the stack of one workgroup: (node name, box bound) per level, level-major so that a wave's accesses are consecutive
inline size_t stack_bytes(int height) { return (size_t)kBlock * (size_t)(height > 0 ? height : 1) * sizeof(uint2); }

struct PointWork {
    const float4 *points;   // (p, max_dist2)
    float4 *out;            // 2 per point: (q, dist2), (u, v, triangle bits, region bits)
    uint64_t count;
    uint64_t first;         // this launch's first point
    DeviceCounters *counters;
};

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
