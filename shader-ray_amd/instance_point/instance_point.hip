// instance_point.hip -- include/shader_ray_instance_point.h: the nearest surface point of a set of placed scenes to each
// world-space point, and the instance it lies on.
//
// One lane per point in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level); a node is entered when any lane's box bound of its stored box
// is not above that lane's best dist2, the nearer child first by the first entering lane's bounds.  At a leaf the instance is
// wave-uniform: its forward map's three rows and the member's SceneView come in by scalar loads, and the lanes whose bound
// passes run the closest-point walk of that member's packed tree (point/point_walk.h's loop) with every box replaced by its
// image box under the map and every triangle's corners mapped before closest_on_triangle.  A lane's best carries from one
// instance into the next, with (instance, triangle) deciding a tie.  The image boxes and their bound are
// instance/image_box.h's, which the other instanced walks over a member's packed tree compile too; the corner mapping stays
// spelled out in this walk, whose register allocation changes when it goes through that header's.
// This library is built apart from libshray_hip.so, libshray_instance.so and libshray_point.so, so their code objects do not
// change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "closest_on_triangle.h"
#include "enter_set.h"
#include "image_box.h"
#include "packed_walk.h"
#include "shader_ray_instance_point.h"
#include "top_level.h"
#include "trace_common.h"

using namespace shray;

namespace {

struct SetWork {
    const float4 *points;   // (p, max_dist2), world space
    float4 *out;            // 2 per point: (q, dist2), (u, v, triangle bits, region bits)
    int32_t *instances;     // one per point, or nullptr
    uint64_t count;
    uint64_t first;         // this launch's first point
    int32_t stack_levels;   // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    DeviceCounters *counters;
};

// a lane's answer so far
struct Best {
    float dist2;   // max_dist2 until a pair qualifies
    int tri, inst;
    Closest found;
};

// One lane's walk of instance `inst`: point_walk.h's loop over the member's packed tree, on image boxes and mapped corners.
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], int inst, const float p[3], uint2 *column,
                                              Best &best, unsigned int &nodes, unsigned int &leaves, unsigned int &tests)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    Record cur = load_record(copy, sc.packed_root);
    nodes++;
    int sp = 0;
    bool go = !(image_bound(m, p, cur.box) > best.dist2);
    while (go) {
        if (cur.b & kLeafFlag) {
            leaves++;
            const uint32_t first = cur.a, n = cur.b & ~kLeafFlag;
            for (uint32_t t = first; t < first + n; t++) {
                tests++;
                const float *v = sc.positions + 9ull * t;
                float c9[9];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const V3 corner = mk(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
#pragma unroll
                    for (int r = 0; r < 3; r++)
                        c9[3 * k + r] = object_row(m[r], corner, true);
                }
                const Closest c = closest_on_triangle(p, c9);
                const bool better = best.tri < 0 ? c.dist2 <= best.dist2
                                                 : (c.dist2 < best.dist2 ||
                                                    (c.dist2 == best.dist2 && (inst < best.inst || (inst == best.inst && (int)t < best.tri))));
                if (better) {
                    best.dist2 = c.dist2;
                    best.tri = (int)t;
                    best.inst = inst;
                    best.found = c;
                }
            }
        } else {
            const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
            const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
            const float lb0 = image_bound(m, p, r0.box), lb1 = image_bound(m, p, r1.box);
            nodes += 2;
            const bool second = lb1 < lb0;   // the nearer child first
            const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
            if (!(near_lb > best.dist2)) {
                if (!(far_lb > best.dist2)) {
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
            if (!(__uint_as_float(e.y) > best.dist2)) {
                cur = load_record(copy, e.x);
                go = true;
                break;
            }
        }
    }
}

// One lane per point.  COUNT: the counting instance.  The pointers are __restrict__ so that a leaf's record, its map and its
// SceneView come in by scalar loads.
template <bool COUNT>
__global__ void __launch_bounds__(kBlock) instance_closest_kernel(SetWork w, const TopNode *__restrict__ nodes,
                                                                  const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                                  const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint2 stack[];
    uint2 *column = stack + threadIdx.x;                                                       // (node name, bound), level-major
    uint32_t *top = reinterpret_cast<uint32_t *>(stack + (size_t)kBlock * w.stack_levels);     // the wave's top-level stack
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 in = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (live)
        in = w.points[index];
    const float p[3] = {in.x, in.y, in.z};
    const bool walk = live && __builtin_isfinite(in.x) && __builtin_isfinite(in.y) && __builtin_isfinite(in.z) && in.w >= 0.0f;

    Best best;
    best.dist2 = in.w;
    best.tri = SHRAY_HIT_MISS;
    best.inst = -1;
    best.found.q[0] = p[0], best.found.q[1] = p[1], best.found.q[2] = p[2];
    best.found.u = 0.0f, best.found.v = 0.0f, best.found.region = SHRAY_REGION_NONE;
    unsigned int visited = 0, leaves = 0, tests = 0, walks = 0;

    if (__builtin_amdgcn_ballot_w64(walk)) {
        walk_top_level(
            nodes, top,
            // The stored box holds every fp32 world corner below it, so its bound is never above a pair's dist2; no
            // ray-origin pad here.
            [&](uint32_t node, const float4 &a, const float4 &b) {
                const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
                return walk && (node == 0u || !(box_bound(p, lo, hi) > best.dist2));
            },
            // the nearer child first by the first entering lane's bounds (the walk's order affects its speed only)
            [&](uint32_t, uint32_t left, unsigned long long entering) {
                const float4 la = reinterpret_cast<const float4 *>(nodes)[2u * left], lb = reinterpret_cast<const float4 *>(nodes)[2u * left + 1u];
                const float4 ra = reinterpret_cast<const float4 *>(nodes)[2u * left + 2u], rb = reinterpret_cast<const float4 *>(nodes)[2u * left + 3u];
                const float llo[3] = {la.x, la.y, la.z}, lhi[3] = {lb.x, lb.y, lb.z}, rlo[3] = {ra.x, ra.y, ra.z}, rhi[3] = {rb.x, rb.y, rb.z};
                const int mine = box_bound(p, rlo, rhi) < box_bound(p, llo, lhi) ? 1 : 0;
                return __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(entering)) == 0;
            },
            [&](int inst, bool enters) {
                const float4 *row = maps + 3u * (uint32_t)inst;
                const float4 m[3] = {row[0], row[1], row[2]};
                const SceneView &sc = leaf_view(records, views, inst);
                if (enters) {
                    walks++;
                    instance_walk(sc, m, inst, p, column, best, visited, leaves, tests);
                }
            });
    }
    if (live) {
        const bool hit = best.tri >= 0;
        w.out[2 * index] = make_float4(best.found.q[0], best.found.q[1], best.found.q[2], hit ? best.dist2 : in.w);
        w.out[2 * index + 1] = make_float4(best.found.u, best.found.v, __int_as_float(best.tri), __int_as_float(best.found.region));
        if (w.instances)
            w.instances[index] = best.inst;
    }
    if (COUNT) {   // (every lane of the wave is here)
        const unsigned long long s0 = wave_sum(visited), s1 = wave_sum(leaves), s2 = wave_sum(tests), s3 = wave_sum(walks);
        if (threadIdx.x == 0) {
            DeviceCounters *c = &w.counters[blockIdx.x % kCounterShards];
            atomicAdd(&c->node_visits, s0);
            atomicAdd(&c->leaf_visits, s1);
            atomicAdd(&c->triangle_tests, s2);
            atomicAdd(&c->traversals, s3);
        }
    }
}

int closest_device(shray_instance_set *set, const shray_point *d_points, int64_t count, shray_closest *d_out, int32_t *d_instances,
                   hipStream_t stream, DeviceCounters *d_counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!set || !d_points || !d_out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, points or out is NULL");
    if (!aligned(d_points, 16) || !aligned(d_out, 16) || !aligned(d_instances, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "point and record buffers must be 16-byte aligned, the instance buffer 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    // (one record per point, kept in registers: K is 0 to walk_set, which then takes no scratch)
    return walk_set(set, true, 0, count, d_instances, stream, [&](const SetWalk &s) {
        SetWork w{(const float4 *)d_points, (float4 *)d_out, s.instances, (uint64_t)count, 0, s.levels, d_counters};
        const size_t lds = s.lds(sizeof(uint2));
        const uint64_t blocks = ((uint64_t)count + kBlock - 1) / kBlock;
        return for_each_launch(blocks, kPointsPerLaunch / kBlock, [&](uint64_t first, dim3 grid) {
            w.first = first * kBlock;
            if (d_counters)
                hipLaunchKernelGGL(instance_closest_kernel<true>, grid, dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
            else
                hipLaunchKernelGGL(instance_closest_kernel<false>, grid, dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
            return launched("instanced closest-point");
        });
    });
}

// the blocking forms: the points to the device, the query on the null stream, the records, instances (and tallies) back
int closest_host(shray_instance_set *set, const shray_point *points, int64_t count, shray_closest *out, int32_t *instances,
                 shray_counters *counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!set || !points || (!out && !counters))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, points or out is NULL");
    if (counters) {
        memset(counters, 0, sizeof(*counters));
        counters->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    if (const int rc = enter_set(set))   // (the errors of a set come before any allocation)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{out, n * sizeof(shray_closest)}, {instances, instances ? n * sizeof(int32_t) : 0}},
                        counters, [&](DeviceBuffer *d_points, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return closest_device(set, d_points->as<const shray_point>(), count, d_out[0].as<shray_closest>(),
                                                  d_out[1].as<int32_t>(), nullptr, shards);
                        });
}

}   // namespace

extern "C" {

int shray_closest_points_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, shray_closest *d_out,
                                          int32_t *d_instances, void *hip_stream)
{
    return closest_device(set, d_points, count, d_out, d_instances, (hipStream_t)hip_stream, nullptr);
}

int shray_closest_points_instances(shray_instance_set *set, const shray_point *points, int64_t count, shray_closest *out,
                                   int32_t *instances)
{
    if (!out && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "out is NULL");
    return closest_host(set, points, count, out, instances, nullptr);
}

int shray_closest_points_instances_counters(shray_instance_set *set, const shray_point *points, int64_t count, shray_closest *out,
                                            int32_t *instances, shray_counters *counters)
{
    if (!counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return closest_host(set, points, count, out, instances, counters);
}

}   // extern "C"
