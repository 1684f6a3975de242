// instance_near.hip -- include/shader_ray_instance_near.h: every triangle of every instance of a set of placed scenes within
// a radius of each world-space point, counted, the nearest K kept in order with their instances.
//
// One lane per point in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level, with the instanced closest-point query's enter predicate and child order, instance_point/
// instance_point.hip); where that query compares a bound with the lane's best dist2, this one compares it with the lane's
// reach: max_dist2, or, in the form that is not asked for counts, the K-th smallest dist2 it holds.  At a leaf the instance is
// wave-uniform: its forward map's three rows and the member's SceneView come in by scalar loads, and the entering lanes run
// the within-radius walk of near/near.hip over that member's packed tree with every box replaced by its image box under the
// map and every triangle's corners mapped before closest_on_triangle.  A lane's K best carry from one instance into the
// next under the key (dist2, instance, triangle).
//
// The K best are kept as near.hip keeps them: their keys in registers for K <= 8 (three words a slot, every index a
// compile-time constant, no scratch), the winners' records computed again at the end by the same function on the same mapped
// corners (the winners' instances are not wave-uniform, so the map and the positions then come by per-lane loads); for
// larger K the whole records are inserted into the point's own K output slots and the instances into the instance buffer.
// The image boxes, their bound and the corner mapping are instance/image_box.h's: this library compiles the code that
// libshray_instance_point.so compiles.  It is built apart from libshray_hip.so and libshray_instance.so, so their code objects
// do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "closest_on_triangle.h"
#include "enter_set.h"
#include "first_k_query.h"
#include "image_box.h"
#include "packed_walk.h"
#include "shader_ray_instance_near.h"
#include "top_level.h"
#include "trace_common.h"

using namespace shray;

// The stack's entries: (node name, image-box bound), 8 bytes, as the instanced closest-point walk's (0), or the name alone,
// 4 bytes, the bound computed again from the node's record when it is popped (1), as near.hip ships.  A bound here costs six
// object_row evaluations, and still (1) is the faster in 22 of 24 measured cells: (1) ships.
#ifndef SHRAY_INSTANCE_NEAR_NAME_STACK
#define SHRAY_INSTANCE_NEAR_NAME_STACK 1
#endif

namespace {

#if SHRAY_INSTANCE_NEAR_NAME_STACK
using StackEntry = uint32_t;
#else
using StackEntry = uint2;
#endif

struct SetNearWork {
    const float4 *points;   // (p, max_dist2), world space
    float4 *out;            // 2 * k per point: (q, dist2), (u, v, triangle bits, region bits); not touched when k == 0
    int32_t *instances;     // k per point, or nullptr (never nullptr for the form that keeps its K best in memory, k > 0)
    int32_t *counts;        // one per point, or nullptr
    uint64_t count;
    uint64_t first;         // this launch's first point
    int32_t k;              // records per point
    int32_t stack_levels;   // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    DeviceCounters *counters;
};

// the key of the header: dist2 as a float comparison, then the instance, then the triangle; an empty slot (triangle < 0) is
// after every member of the near set
__device__ __forceinline__ bool before(float d, int inst, int tri, float slot_d, int slot_inst, int slot_tri)
{
    return slot_tri < 0 || d < slot_d || (d == slot_d && (inst < slot_inst || (inst == slot_inst && tri < slot_tri)));
}

// the record of the pair (the instance whose map is m, triangle t of its scene): the corners mapped, then the closest point
__device__ __forceinline__ Closest closest_on_mapped(const float4 (&m)[3], const float *positions, uint32_t t, const float p[3])
{
    return with_mapped_corners(m, positions, t, [&](const float *c9) { return closest_on_triangle(p, c9); });
}

// A lane's K best.  SLOTS > 0: the keys in registers; kSlotsInMemory: the records in the point's own output slots and
// their instances beside them (any k, also 0).
template <int SLOTS>
struct Held {
    static constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float d[R];   // (plain scalars: every index is a constant once unrolled)
    int inst[R], tri[R];
    float4 *slots;       // in memory: this point's own records and instances (dereferenced only when live and k > 0)
    int32_t *slot_inst;
    int k;

    // the key moves in where it sorts, the rest move down, the last falls off; returns the dist2 of slot k - 1 afterwards
    // when PRUNE (an empty slot holds max_dist2), else `reach` as it was
    template <bool PRUNE>
    __device__ __forceinline__ float insert(const Closest &c, int in, int t, float reach)
    {
        const float dist2 = c.dist2;
        if (SLOTS != kSlotsInMemory) {
#pragma unroll
            for (int i = R - 1; i >= 0; i--) {
                constexpr int kNone = 0;
                const int up = i > 0 ? i - 1 : kNone;
                const bool here = before(dist2, in, t, d[i], inst[i], tri[i]);
                const bool above = i > 0 && before(dist2, in, t, d[up], inst[up], tri[up]);
                d[i] = above ? d[up] : (here ? dist2 : d[i]);
                inst[i] = above ? inst[up] : (here ? in : inst[i]);
                tri[i] = above ? tri[up] : (here ? t : tri[i]);
            }
            if (PRUNE) {
#pragma unroll
                for (int i = 0; i < R; i++)
                    reach = i == k - 1 ? d[i] : reach;
            }
        } else if (k > 0 && before(dist2, in, t, slots[2 * (k - 1)].w, slot_inst[k - 1], __float_as_int(slots[2 * (k - 1) + 1].z))) {
            int i = k - 1;
            while (i > 0) {
                const float4 s0 = slots[2 * (i - 1)], s1 = slots[2 * (i - 1) + 1];
                const int si = slot_inst[i - 1];
                if (!before(dist2, in, t, s0.w, si, __float_as_int(s1.z)))
                    break;
                slots[2 * i] = s0, slots[2 * i + 1] = s1;
                slot_inst[i] = si;
                i--;
            }
            slots[2 * i] = make_float4(c.q[0], c.q[1], c.q[2], dist2);
            slots[2 * i + 1] = make_float4(c.u, c.v, __int_as_float(t), __int_as_float(c.region));
            slot_inst[i] = in;
            if (PRUNE)
                reach = slots[2 * (k - 1)].w;   // (a miss record holds max_dist2)
        }
        return reach;
    }
};

// One lane's walk of instance `inst`: near.hip's loop over the member's packed tree, on image boxes and mapped corners.
template <int SLOTS, bool PRUNE>
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], int inst, const float p[3], float md,
                                              StackEntry *column, Held<SLOTS> &held, float &reach, int &n, unsigned int &nodes,
                                              unsigned int &leaves, unsigned int &tests)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    Record cur = load_record(copy, sc.packed_root);
    nodes++;
    int sp = 0;
    bool go = !(image_bound(m, p, cur.box) > reach);
    while (go) {
        if (cur.b & kLeafFlag) {
            leaves++;
            const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
            for (uint32_t t = first; t < first + in_leaf; t++) {
                tests++;
                const Closest c = closest_on_mapped(m, sc.positions, t, p);
                if (!(c.dist2 <= md))
                    continue;
                n++;
                reach = held.template insert<PRUNE>(c, inst, (int)t, reach);
            }
        } else {
            const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
            const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
            const float lb0 = image_bound(m, p, r0.box), lb1 = image_bound(m, p, r1.box);
            nodes += 2;
            const bool second = lb1 < lb0;   // the nearer child first
            const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
            if (!(near_lb > reach)) {
                if (!(far_lb > reach)) {
#if SHRAY_INSTANCE_NEAR_NAME_STACK
                    column[(size_t)sp * kBlock] = second ? n0 : n1;
#else
                    column[(size_t)sp * kBlock] = make_uint2(second ? n0 : n1, __float_as_uint(far_lb));
#endif
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
#if SHRAY_INSTANCE_NEAR_NAME_STACK
            cur = load_record(copy, column[(size_t)sp * kBlock]);
            if (PRUNE && image_bound(m, p, cur.box) > reach)   // the reach has dropped below it since the push
                continue;
            go = true;
            break;
#else
            const uint2 e = column[(size_t)sp * kBlock];
            if (PRUNE && __uint_as_float(e.y) > reach)   // the reach has dropped below it since the push
                continue;
            cur = load_record(copy, e.x);
            go = true;
            break;
#endif
        }
    }
}

// One lane per point.  SLOTS, PRUNE, COUNT: as near_kernel's (near/near.hip).  The pointers are __restrict__ so that a leaf's
// record, its map and its SceneView come in by scalar loads.
template <int SLOTS, bool PRUNE, bool COUNT>
__global__ void __launch_bounds__(kBlock) instance_near_kernel(SetNearWork w, const TopNode *__restrict__ nodes,
                                                               const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                               const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) StackEntry near_stack[];
    StackEntry *column = near_stack + threadIdx.x;                                                    // level-major
    uint32_t *top = reinterpret_cast<uint32_t *>(near_stack + (size_t)kBlock * w.stack_levels);       // the wave's top-level stack
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 in = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (live)
        in = w.points[index];
    const float p[3] = {in.x, in.y, in.z};
    const float md = in.w;
    const bool walk = live && __builtin_isfinite(in.x) && __builtin_isfinite(in.y) && __builtin_isfinite(in.z) && md >= 0.0f;
    const int k = w.k;
    const float4 miss0 = make_float4(p[0], p[1], p[2], md);
    const float4 miss1 = make_float4(0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS), __int_as_float(SHRAY_REGION_NONE));

    Held<SLOTS> held;
    held.k = k;
    held.slots = w.out + 2ull * (index * (uint64_t)k);        // this point's own (dereferenced only when live and k > 0)
    held.slot_inst = w.instances + index * (uint64_t)k;
#pragma unroll
    for (int i = 0; i < Held<SLOTS>::R; i++)
        held.d[i] = md, held.inst[i] = -1, held.tri[i] = SHRAY_HIT_MISS;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            held.slots[2 * i] = miss0, held.slots[2 * i + 1] = miss1, held.slot_inst[i] = -1;
    // what a bound must not exceed: max_dist2, or (PRUNE) the k-th smallest dist2 held, max_dist2 while fewer are held
    float reach = md;
    int n = 0;
    unsigned int visited = 0, leaves = 0, tests = 0, walks = 0;

    if (__builtin_amdgcn_ballot_w64(walk)) {
        walk_top_level(
            nodes, top,
            // The stored box holds every fp32 world corner below it, so its bound is never above a pair's dist2; a bound that
            // equals the reach enters (a lower instance wins a tie there).  The root is not tested.
            [&](uint32_t node, const float4 &a, const float4 &b) {
                const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
                return walk && (node == 0u || !(box_bound(p, lo, hi) > reach));
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
                    instance_walk<SLOTS, PRUNE>(sc, m, inst, p, md, column, held, reach, n, visited, leaves, tests);
                }
            });
    }
    if (live) {
        if (SLOTS != kSlotsInMemory) {
            // the winners' records, by the function and the inputs that gave their keys; the head slot is read and the rest
            // move up, so that every index stays a constant.  A winner's map and positions come by this lane's own loads.
            int32_t *instances = w.instances ? held.slot_inst : nullptr;
#pragma nounroll
            for (int i = 0; i < k; i++) {
                const int tri = held.tri[0], inst = held.inst[0];
#pragma unroll
                for (int j = 0; j + 1 < Held<SLOTS>::R; j++)
                    held.tri[j] = held.tri[j + 1], held.inst[j] = held.inst[j + 1];
                float4 a = miss0, b = miss1;
                if (tri >= 0) {
                    const float4 *row = maps + 3u * (uint32_t)inst;
                    const float4 m[3] = {row[0], row[1], row[2]};
                    const Closest c = closest_on_mapped(m, leaf_view(records, views, inst).positions, (uint32_t)tri, p);
                    a = make_float4(c.q[0], c.q[1], c.q[2], c.dist2);
                    b = make_float4(c.u, c.v, __int_as_float(tri), __int_as_float(c.region));
                }
                held.slots[2 * i] = a, held.slots[2 * i + 1] = b;
                if (instances)
                    instances[i] = inst;
            }
        }
        if (w.counts)
            w.counts[index] = n;
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

constexpr Nouns kNouns = {"point", "points", "set", "out", "max_near", "instanced within-radius query"};

// include/shader_ray_near.h's params check (near/near.hip makes the same one)
int check_params(const shray_near_params *np)
{
    if (!np)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "near params are NULL");
    if (np->struct_size != sizeof(shray_near_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_near_params.struct_size is %u, this library expects %zu", np->struct_size,
                    sizeof(shray_near_params));
    if (np->max_near < 0 || np->max_near > SHRAY_NEAR_MAX || np->reserved[0] != 0 || np->reserved[1] != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "near params out of range (max_near %d of 0 .. %d, reserved %d, %d)", np->max_near,
                    (int)SHRAY_NEAR_MAX, np->reserved[0], np->reserved[1]);
    return SHRAY_OK;
}

// the checks every form makes before it touches a set or a device
int check_query(shray_instance_set *set, const shray_near_params *np, const void *points, int64_t count, const void *out,
                const void *counts)
{
    const int rc = check_params(np);
    return rc ? rc : check_first_k(kNouns, set, points, count, np->max_near, out, counts);
}

int near_device(shray_instance_set *set, const shray_near_params *np, const shray_point *d_points, int64_t count, shray_closest *d_out,
                int32_t *d_instances, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(set, np, d_points, count, d_out, d_counts);
    if (rc)
        return rc;
    const int k = np->max_near;
    if (!aligned(d_points, 16) || (k > 0 && !aligned(d_out, 16)) || !aligned(d_instances, 4) || !aligned(d_counts, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT,
                    "point and record buffers must be 16-byte aligned, the instances and counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    return walk_set(set, true, k, count, d_instances, stream, [&](const SetWalk &s) {
        SetNearWork w{(const float4 *)d_points, k > 0 ? (float4 *)d_out : nullptr, k > 0 ? s.instances : nullptr, d_counts, (uint64_t)count, 0,
                      k, s.levels, d_counters};
        const size_t lds = s.lds(sizeof(StackEntry));
        return first_k_launches(kNouns, w, count, [&](dim3 grid) {
            with_slots(k, [&](auto slots) {
                with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                    hipLaunchKernelGGL((instance_near_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value>), grid,
                                       dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
                });
            });
        });
    });
}

// the blocking forms: the points to the device, the query on the null stream, the records, instances, counts (and tallies) back
int near_host(shray_instance_set *set, const shray_near_params *np, const shray_point *points, int64_t count, shray_closest *out,
              int32_t *instances, int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(set, np, points, count, out, counts))
        return rc;
    return first_k_blocking(
        {points, sizeof(shray_point), out, sizeof(shray_closest), instances, counts}, count, np->max_near, tallies,
        [&] { return enter_set(set); },
        [&](void *d_points, void *d_out, int32_t *d_instances, int32_t *d_counts, DeviceCounters *shards) {
            return near_device(set, np, (const shray_point *)d_points, count, (shray_closest *)d_out, d_instances, d_counts, nullptr, shards);
        });
}

}   // namespace

static_assert(sizeof(shray_near_params) == 16, "shray_near_params is 16 bytes");
static_assert(sizeof(shray_point) == 16 && sizeof(shray_closest) == 32, "the closest-point query's records");

extern "C" {

int shray_near_triangles_instances_device(shray_instance_set *set, const shray_near_params *np, const shray_point *d_points,
                                          int64_t count, shray_closest *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return near_device(set, np, d_points, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_near_triangles_instances(shray_instance_set *set, const shray_near_params *np, const shray_point *points, int64_t count,
                                   shray_closest *out, int32_t *instances, int32_t *counts)
{
    return near_host(set, np, points, count, out, instances, counts, nullptr);
}

int shray_near_triangles_instances_counters(shray_instance_set *set, const shray_near_params *np, const shray_point *points,
                                            int64_t count, shray_closest *out, int32_t *instances, int32_t *counts,
                                            shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : near_host(set, np, points, count, out, instances, counts, counters);
}

}   // extern "C"
