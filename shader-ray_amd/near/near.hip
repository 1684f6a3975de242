// near.hip -- include/shader_ray_near.h: every triangle of a resident scene within a radius of each caller-supplied point,
// counted, the nearest K kept in order.
//
// One lane per point in one-wave workgroups.  The walk is shaped as the closest-point walk (point/point_walk.h; the box bound
// and closest_on_triangle both call are point/closest_on_triangle.h: a record here is that function's, not a copy's): the 32-byte records of
// octant copy 7 of the packed tree, the corners from the scene's positions, a stack in LDS, level-major, one entry per edge
// of the tree's height, nearest child first.  The near set does not depend on the visit order (the header).  The form that is
// asked for counts skips a node only when its box bound is above max_dist2; the form that is not skips one whose bound is
// above the K-th smallest dist2 held: nothing below it can enter the nearest K.
//
// The K best are kept by sorted insertion of their keys (dist2, triangle): in registers for K <= 8 (instances for 1, 2, 4 and
// 8 slots; every index is a compile-time constant, so there is no scratch), and the winners' records are computed again at the
// end by the same function on the same inputs, which gives the same bits.  For larger K the whole records are inserted into
// the point's own K output slots.
// This library is built apart from libshray_hip.so, so the renderer's code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "client_internal.h"
#include "closest_on_triangle.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "shader_ray_near.h"

using namespace shray;

// The stack's entries: (node name, box bound), 8 bytes, as the closest-point walk's (0), or the name alone, 4 bytes, the bound
// computed again from the node's record when it is popped (1).  DESIGN section 15 has both measured; the faster one, (1), ships.
#ifndef SHRAY_NEAR_NAME_STACK
#define SHRAY_NEAR_NAME_STACK 1
#endif

namespace {

#if SHRAY_NEAR_NAME_STACK
using StackEntry = uint32_t;
#else
using StackEntry = uint2;
#endif

struct NearWork {
    const float4 *points;   // (p, max_dist2)
    float4 *out;            // 2 * k per point: (q, dist2), (u, v, triangle bits, region bits); not touched when k == 0
    int32_t *counts;        // one per point, or nullptr
    uint64_t count;
    uint64_t first;         // this launch's first point
    int32_t k;              // records per point
    DeviceCounters *counters;
};

// the key of the header: dist2 as a float comparison, then the triangle index; an empty slot (triangle < 0) is after every
// member of the near set
__device__ __forceinline__ bool before(float d, int tri, float slot_d, int slot_tri)
{
    return slot_tri < 0 || d < slot_d || (d == slot_d && tri < slot_tri);
}

// One lane per point.  SLOTS: the register slots of the K best keys (k <= SLOTS), kSlotsInMemory: the records live in the
// point's output slots (any k, also 0).  PRUNE: skip nodes that cannot reach the nearest k (no count is written).  COUNT: the
// work counters.
template <int SLOTS, bool PRUNE, bool COUNT>
__global__ void __launch_bounds__(kBlock) near_kernel(SceneView sc, NearWork w)
{
    extern __shared__ __attribute__((aligned(16))) StackEntry near_stack[];
    StackEntry *column = near_stack + threadIdx.x;   // level-major: a wave's accesses are consecutive
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
    float4 *slots = w.out + 2ull * (index * (uint64_t)k);   // this point's own (dereferenced only when live and k > 0)

    constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float held_d[R];   // (plain scalars: every index below is a constant once unrolled)
    int held_t[R];
#pragma unroll
    for (int i = 0; i < R; i++)
        held_d[i] = md, held_t[i] = SHRAY_HIT_MISS;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            slots[2 * i] = miss0, slots[2 * i + 1] = miss1;
    // what a node's bound must not exceed: max_dist2, or (PRUNE) the k-th smallest dist2 held, max_dist2 while fewer are held
    float reach = md;
    int n = 0;
    unsigned int nodes = 0, leaves = 0, tests = 0;

    if (walk) {
        const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
        Record cur = load_record(copy, sc.packed_root);
        nodes++;
        int sp = 0;
        bool go = !(box_bound(p, cur.box.lo, cur.box.hi) > reach);
        while (go) {
            if (cur.b & kLeafFlag) {
                leaves++;
                const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
                for (uint32_t t = first; t < first + in_leaf; t++) {
                    tests++;
                    const Closest c = closest_on_triangle(p, sc.positions + 9ull * t);
                    if (!(c.dist2 <= md))
                        continue;
                    const float d = c.dist2;
                    const int tri = (int)t;
                    n++;
                    if (SLOTS != kSlotsInMemory) {
                        // the key moves in where it sorts, the rest move down, the last falls off
#pragma unroll
                        for (int i = R - 1; i >= 0; i--) {
                            constexpr int kNone = 0;
                            const int up = i > 0 ? i - 1 : kNone;
                            const bool here = before(d, tri, held_d[i], held_t[i]);
                            const bool above = i > 0 && before(d, tri, held_d[up], held_t[up]);
                            held_d[i] = above ? held_d[up] : (here ? d : held_d[i]);
                            held_t[i] = above ? held_t[up] : (here ? tri : held_t[i]);
                        }
                        if (PRUNE) {
#pragma unroll
                            for (int i = 0; i < R; i++)
                                reach = i == k - 1 ? held_d[i] : reach;   // (an empty slot holds max_dist2)
                        }
                    } else if (k > 0 && before(d, tri, slots[2 * (k - 1)].w, __float_as_int(slots[2 * (k - 1) + 1].z))) {
                        int i = k - 1;
                        while (i > 0) {
                            const float4 s0 = slots[2 * (i - 1)], s1 = slots[2 * (i - 1) + 1];
                            if (!before(d, tri, s0.w, __float_as_int(s1.z)))
                                break;
                            slots[2 * i] = s0, slots[2 * i + 1] = s1;
                            i--;
                        }
                        slots[2 * i] = make_float4(c.q[0], c.q[1], c.q[2], d);
                        slots[2 * i + 1] = make_float4(c.u, c.v, __int_as_float(tri), __int_as_float(c.region));
                        if (PRUNE)
                            reach = slots[2 * (k - 1)].w;   // (a miss record holds max_dist2)
                    }
                }
            } else {
                const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
                const float lb0 = box_bound(p, r0.box.lo, r0.box.hi), lb1 = box_bound(p, r1.box.lo, r1.box.hi);
                nodes += 2;
                const bool second = lb1 < lb0;   // the nearer child first
                const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
                if (!(near_lb > reach)) {
                    if (!(far_lb > reach)) {
#if SHRAY_NEAR_NAME_STACK
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
#if SHRAY_NEAR_NAME_STACK
                cur = load_record(copy, column[(size_t)sp * kBlock]);
                if (PRUNE && box_bound(p, cur.box.lo, cur.box.hi) > reach)   // the reach has dropped below it since the push
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
    if (live) {
        if (SLOTS != kSlotsInMemory) {
            // the winners' records, by the function and the inputs that gave their keys; the head slot is read and the rest
            // move up, so that every index stays a constant
#pragma nounroll
            for (int i = 0; i < k; i++) {
                const int tri = held_t[0];
#pragma unroll
                for (int j = 0; j + 1 < R; j++)
                    held_t[j] = held_t[j + 1];
                float4 a = miss0, b = miss1;
                if (tri >= 0) {
                    const Closest c = closest_on_triangle(p, sc.positions + 9ull * (uint32_t)tri);
                    a = make_float4(c.q[0], c.q[1], c.q[2], c.dist2);
                    b = make_float4(c.u, c.v, __int_as_float(tri), __int_as_float(c.region));
                }
                slots[2 * i] = a, slots[2 * i + 1] = b;
            }
        }
        if (w.counts)
            w.counts[index] = n;
    }
    if (COUNT) {
        const unsigned long long s0 = wave_sum(nodes), s1 = wave_sum(leaves), s2 = wave_sum(tests);   // (every lane is here)
        if (threadIdx.x == 0) {
            DeviceCounters *c = &w.counters[blockIdx.x % kCounterShards];
            atomicAdd(&c->node_visits, s0);
            atomicAdd(&c->leaf_visits, s1);
            atomicAdd(&c->triangle_tests, s2);
        }
    }
}

constexpr Nouns kNouns = {"point", "points", "scene", "out", "max_near", "within-radius query"};

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

// the checks every form makes before it touches a scene or a device
int check_query(shray_scene *scene, const shray_near_params *np, const void *points, int64_t count, const void *out, const void *counts)
{
    const int rc = check_params(np);
    return rc ? rc : check_first_k(kNouns, scene, points, count, np->max_near, out, counts);
}

int near_device(shray_scene *scene, const shray_near_params *np, const shray_point *d_points, int64_t count, shray_closest *d_out,
                int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(scene, np, d_points, count, d_out, d_counts);
    if (rc)
        return rc;
    const int k = np->max_near;
    if (!aligned(d_points, 16) || (k > 0 && !aligned(d_out, 16)) || (d_counts && !aligned(d_counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "point and record buffers must be 16-byte aligned, the counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))
        return rc;
    NearWork w{(const float4 *)d_points, k > 0 ? (float4 *)d_out : nullptr, d_counts, (uint64_t)count, 0, k, d_counters};
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(StackEntry);
    return first_k_launches(kNouns, w, count, [&](dim3 grid) {
        with_slots(k, [&](auto slots) {
            with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                hipLaunchKernelGGL((near_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value>), grid, dim3(kBlock), lds,
                                   stream, q.view, w);
            });
        });
    });
}

// the blocking forms: the points to the device, the query on the null stream, the records, counts (and tallies) back
int near_host(shray_scene *scene, const shray_near_params *np, const shray_point *points, int64_t count, shray_closest *out,
              int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(scene, np, points, count, out, counts))
        return rc;
    return first_k_blocking(
        {points, sizeof(shray_point), out, sizeof(shray_closest), nullptr, counts}, count, np->max_near, tallies,
        [&] {
            ShrayQueryScene q;
            int height = 0;
            return enter_walkable_scene(scene, &q, &height);
        },
        [&](void *d_points, void *d_out, int32_t *, int32_t *d_counts, DeviceCounters *shards) {
            return near_device(scene, np, (const shray_point *)d_points, count, (shray_closest *)d_out, d_counts, nullptr, shards);
        });
}

}   // namespace

static_assert(sizeof(shray_near_params) == 16, "shray_near_params is 16 bytes");
static_assert(sizeof(shray_point) == 16 && sizeof(shray_closest) == 32, "the closest-point query's records");

extern "C" {

void shray_near_params_init(shray_near_params *np)
{
    if (!np)
        return;
    np->struct_size = sizeof(shray_near_params);
    np->max_near = 8;
    np->reserved[0] = np->reserved[1] = 0;
}

int shray_near_triangles_device(shray_scene *scene, const shray_near_params *np, const shray_point *d_points, int64_t count,
                                shray_closest *d_out, int32_t *d_counts, void *hip_stream)
{
    return near_device(scene, np, d_points, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_near_triangles(shray_scene *scene, const shray_near_params *np, const shray_point *points, int64_t count, shray_closest *out,
                         int32_t *counts)
{
    return near_host(scene, np, points, count, out, counts, nullptr);
}

int shray_near_triangles_counters(shray_scene *scene, const shray_near_params *np, const shray_point *points, int64_t count,
                                  shray_closest *out, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : near_host(scene, np, points, count, out, counts, counters);
}

}   // extern "C"
