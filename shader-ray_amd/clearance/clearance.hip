// clearance.hip -- include/shader_ray_clearance.h: every triangle of a resident scene within a squared distance of each query
// triangle, counted, the nearest K kept in order, each with its dist2 and a witness on either triangle.
// The queries are caller-supplied triangles or the scene's own.
//
// One lane per query in one-wave workgroups.  The walk is near/near.hip's with a box for the point: the 32-byte records of
// octant copy 7 of the packed tree (point/packed_walk.h), the corners from the scene's positions, a level-major LDS column of
// node names, one entry per edge of the tree's height, both children loaded and bounded, the nearer first, the farther pushed
// if it is in reach, a popped node's bound computed again.  A node is skipped only when the squared gap between its box and the
// query's vertex box is above the reach: max_dist2 in the forms that count, the K-th smallest dist2 held in the form that does
// not.  The bound never exceeds a pair's dist2 (the header), so the set does not depend on the visit order.  The same bound on a
// triangle's own vertex box skips a pair before its arithmetic.
//
// The K best are kept by sorted insertion of their keys (dist2, triangle): in registers for K <= 8 (instances for 1, 2, 4 and
// 8 slots; every index is a compile-time constant), and the winners' records are computed again at the end by the same
// function on the same inputs, which gives the same bits.  For larger K the whole records are inserted into the query's own
// K output slots.  The per-pair arithmetic is point/triangle_pair_distance.h's, which a later instanced form compiles too.
// Where a query's nine floats come from and whether triangles that share a corner are skipped are wave-uniform runtime
// branches on the launch's arguments, as in intersect/intersect.hip.
// This library is built apart from libshray_hip.so, so the renderer's and the other clients' code objects do not change.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "client_internal.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "params_check.h"
#include "shader_ray_clearance.h"
#include "triangle_pair_distance.h"

using namespace shray;

namespace {

struct ClearanceWork {
    const float4 *triangles;   // three per query: (a, pad), (b, pad), (c, pad); nullptr: the scene's own triangles
    float4 *out;               // 3 * k per query: (x, dist2), (y, triangle bits), (feature bits, 0, 0, 0); not touched when k == 0
    int32_t *counts;           // one per query, or nullptr
    uint64_t count;
    uint64_t first;            // this launch's first query
    uint64_t self_first;       // the scene triangle of query 0 (the self form)
    int32_t k;                 // records per query
    uint32_t skip_shared;      // SHRAY_CLEARANCE_SKIP_SHARED is set
    float max_dist2;
    DeviceCounters *counters;
};

// the key of the header: dist2 as a float comparison, then the triangle index; an empty slot (triangle < 0) is after every
// member
__device__ __forceinline__ bool before(float d, int tri, float slot_d, int slot_tri)
{
    return slot_tri < 0 || d < slot_d || (d == slot_d && tri < slot_tri);
}

__device__ __forceinline__ void store_record(float4 *slot, const PairDistance &r, int tri)
{
    slot[0] = make_float4(r.x[0], r.x[1], r.x[2], r.dist2);
    slot[1] = make_float4(r.y[0], r.y[1], r.y[2], __int_as_float(tri));
    slot[2] = make_float4(__int_as_float(r.feature), 0.0f, 0.0f, 0.0f);
}

// One lane per query.  SLOTS: the register slots of the K best keys (k <= SLOTS), kSlotsInMemory: the records live in the
// query's output slots (any k, also 0).  PRUNE: skip what cannot reach the nearest k (no count is written).  ANY: stop at the
// first member (k is 0).  COUNT: the work counters.
template <int SLOTS, bool PRUNE, bool ANY, bool COUNT>
__global__ void __launch_bounds__(kBlock) clearance_kernel(SceneView sc, ClearanceWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t clearance_stack[];
    uint32_t *column = clearance_stack + threadIdx.x;   // level-major: a wave's accesses are consecutive
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    Query q;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            q.p[i][j] = 0.0f;
    if (live) {
        if (w.triangles) {
            const float4 c0 = w.triangles[3 * index], c1 = w.triangles[3 * index + 1], c2 = w.triangles[3 * index + 2];
            q.p[0][0] = c0.x, q.p[0][1] = c0.y, q.p[0][2] = c0.z;
            q.p[1][0] = c1.x, q.p[1][1] = c1.y, q.p[1][2] = c1.z;
            q.p[2][0] = c2.x, q.p[2][1] = c2.y, q.p[2][2] = c2.z;
        } else {
            const float *own = sc.positions + 9ull * (w.self_first + index);   // (the host checked the range)
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    q.p[i][j] = own[3 * i + j];
        }
    }
    const float md = w.max_dist2;
    const bool walk = make_query(q) && live && md >= 0.0f;   // (a NaN max_dist2 fails the comparison)
    const bool skip_shared = w.skip_shared != 0;
    const int k = w.k;
    const float4 miss0 = make_float4(0.0f, 0.0f, 0.0f, md);
    const float4 miss1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS));
    const float4 miss2 = make_float4(__int_as_float(-1), 0.0f, 0.0f, 0.0f);
    float4 *slots = w.out + 3ull * (index * (uint64_t)k);   // this query's own (dereferenced only when live and k > 0)

    constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float held_d[R];   // (plain scalars: every index below is a constant once unrolled)
    int held_t[R];
#pragma unroll
    for (int i = 0; i < R; i++)
        held_d[i] = md, held_t[i] = SHRAY_HIT_MISS;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            slots[3 * i] = miss0, slots[3 * i + 1] = miss1, slots[3 * i + 2] = miss2;
    // what a bound must not exceed: max_dist2, or (PRUNE) the k-th smallest dist2 held, max_dist2 while fewer are held
    float reach = md;
    int n = 0;
    unsigned int nodes = 0, leaves = 0, tests = 0;

    if (walk) {
        const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
        Record cur = load_record(copy, sc.packed_root);
        nodes++;
        int sp = 0;
        bool go = !(box_gap2(q.lo, q.hi, cur.box.lo, cur.box.hi) > reach);
        while (go) {
            if (cur.b & kLeafFlag) {
                leaves++;
                const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
                for (uint32_t t = first; t < first + in_leaf; t++) {
                    const float *tri = sc.positions + 9ull * t;
                    if (skip_shared && shares_corner(q, tri))
                        continue;
                    if (triangle_gap2(q, tri) > reach)   // the pair's dist2 is no less
                        continue;
                    tests++;
                    const PairDistance c = pair_distance(q, tri);
                    if (!(c.dist2 <= md))
                        continue;
                    n++;
                    if (ANY)
                        break;
                    const float d = c.dist2;
                    const int id = (int)t;
                    if (SLOTS != kSlotsInMemory) {
                        // the key moves in where it sorts, the rest move down, the last falls off
#pragma unroll
                        for (int i = R - 1; i >= 0; i--) {
                            constexpr int kNone = 0;
                            const int up = i > 0 ? i - 1 : kNone;
                            const bool here = before(d, id, held_d[i], held_t[i]);
                            const bool above = i > 0 && before(d, id, held_d[up], held_t[up]);
                            held_d[i] = above ? held_d[up] : (here ? d : held_d[i]);
                            held_t[i] = above ? held_t[up] : (here ? id : held_t[i]);
                        }
                        if (PRUNE) {
#pragma unroll
                            for (int i = 0; i < R; i++)
                                reach = i == k - 1 ? held_d[i] : reach;   // (an empty slot holds max_dist2)
                        }
                    } else if (k > 0 && before(d, id, slots[3 * (k - 1)].w, __float_as_int(slots[3 * (k - 1) + 1].w))) {
                        int i = k - 1;
                        while (i > 0) {
                            const float4 s0 = slots[3 * (i - 1)], s1 = slots[3 * (i - 1) + 1], s2 = slots[3 * (i - 1) + 2];
                            if (!before(d, id, s0.w, __float_as_int(s1.w)))
                                break;
                            slots[3 * i] = s0, slots[3 * i + 1] = s1, slots[3 * i + 2] = s2;
                            i--;
                        }
                        store_record(slots + 3 * i, c, id);
                        if (PRUNE)
                            reach = slots[3 * (k - 1)].w;   // (a miss record holds max_dist2)
                    }
                }
                if (ANY && n > 0)
                    break;
            } else {
                const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
                const float lb0 = box_gap2(q.lo, q.hi, r0.box.lo, r0.box.hi), lb1 = box_gap2(q.lo, q.hi, r1.box.lo, r1.box.hi);
                nodes += 2;
                const bool second = lb1 < lb0;   // the nearer child first
                const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
                if (!(near_lb > reach)) {
                    if (!(far_lb > reach)) {
                        column[(size_t)sp * kBlock] = second ? n0 : n1;
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
                cur = load_record(copy, column[(size_t)sp * kBlock]);
                if (PRUNE && box_gap2(q.lo, q.hi, cur.box.lo, cur.box.hi) > reach)   // the reach has dropped below it since the push
                    continue;
                go = true;
                break;
            }
        }
    }
    if (live) {
        if (SLOTS != kSlotsInMemory) {
            // the winners' records, by the function and the inputs that gave their keys; the head slot is read and the rest
            // move up, so that every index stays a constant
#pragma nounroll
            for (int i = 0; i < k; i++) {
                const int id = held_t[0];
#pragma unroll
                for (int j = 0; j + 1 < R; j++)
                    held_t[j] = held_t[j + 1];
                if (id >= 0)
                    store_record(slots + 3 * i, pair_distance(q, sc.positions + 9ull * (uint32_t)id), id);
                else
                    slots[3 * i] = miss0, slots[3 * i + 1] = miss1, slots[3 * i + 2] = miss2;
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

constexpr Nouns kNouns = {"triangle", "triangles", "scene", "out", "max_pairs", "triangle-distance query"};

// the checks every form makes before it touches a scene or a device; the self form's `triangles` is its scene (it has no
// item array) and its `first` the first of the scene's triangles, 0 for the item forms
int check_query(shray_scene *scene, const shray_clearance_params *op, const void *triangles, int64_t first, int64_t count, const void *out,
                const void *counts)
{
    const int rc = check_params(op);
    if (rc)
        return rc;
    return check_first_k(kNouns, scene, triangles, count, op->max_pairs, out, counts, [&] {
        if (first < 0)
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative first triangle %lld", (long long)first);
        return check_any(op, counts);
    });
}

int check_alignment(const void *triangles, const void *out, const void *counts)
{
    if (!aligned(triangles, 16) || (out && !aligned(out, 16)) || (counts && !aligned(counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the triangles and the records must be 16-byte aligned, the counts 4-byte aligned");
    return SHRAY_OK;
}

// the self form's range against the scene's triangle count: the one refusal that reads the scene
int check_self_range(shray_scene *scene, int64_t first, int64_t count)
{
    ShrayQueryScene q;
    if (const int rc = enter_scene(scene, &q))
        return rc;
    if ((uint64_t)first + (uint64_t)count > q.view.triangle_count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "triangles %lld .. %lld are not all among the scene's %u", (long long)first,
                    (long long)first + (long long)count, q.view.triangle_count);
    return SHRAY_OK;
}

// The device form of both kinds of query: d_triangles, or with self the scene's own triangles [first, first + count).
int clearance_device(shray_scene *scene, const shray_clearance_params *op, bool self, const shray_triangle *d_triangles, int64_t first,
                     int64_t count, shray_pair_distance *d_out, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(scene, op, self ? (const void *)scene : d_triangles, first, count, d_out, d_counts);
    if (rc)
        return rc;
    const int k = op->max_pairs;
    const bool any = (op->flags & SHRAY_CLEARANCE_ANY) != 0;
    if ((rc = check_alignment(self ? nullptr : d_triangles, k > 0 ? d_out : nullptr, d_counts)))
        return rc;
    if (self && (rc = check_self_range(scene, first, count)))
        return rc;
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))
        return rc;
    ClearanceWork w{self ? nullptr : (const float4 *)d_triangles, k > 0 ? (float4 *)d_out : nullptr, d_counts, (uint64_t)count, 0,
                    (uint64_t)first, k, (op->flags & SHRAY_CLEARANCE_SKIP_SHARED) ? 1u : 0u, op->max_dist2, d_counters};
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint32_t);
    return first_k_launches(kNouns, w, count, [&](dim3 grid) {
        if (any && d_counters)
            hipLaunchKernelGGL((clearance_kernel<kSlotsInMemory, false, true, true>), grid, dim3(kBlock), lds, stream, q.view, w);
        else if (any)
            hipLaunchKernelGGL((clearance_kernel<kSlotsInMemory, false, true, false>), grid, dim3(kBlock), lds, stream, q.view, w);
        else
            with_slots(k, [&](auto slots) {
                with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                    hipLaunchKernelGGL((clearance_kernel<decltype(slots)::value, decltype(prune)::value, false, decltype(tally)::value>), grid,
                                       dim3(kBlock), lds, stream, q.view, w);
                });
            });
    });
}

// the blocking forms: the triangles to the device (none for the self form), the query on the null stream, the records,
// counts (and tallies) back
int clearance_host(shray_scene *scene, const shray_clearance_params *op, bool self, const shray_triangle *triangles, int64_t first,
                   int64_t count, shray_pair_distance *out, int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(scene, op, self ? (const void *)scene : triangles, first, count, out, counts))
        return rc;
    if (const int rc = check_alignment(self ? nullptr : triangles, op->max_pairs > 0 ? out : nullptr, counts))
        return rc;
    if (self)
        if (const int rc = check_self_range(scene, first, count))
            return rc;
    static const float no_items[4] = {};
    return first_k_blocking(
        {self ? (const void *)no_items : triangles, self ? 0 : sizeof(shray_triangle), out, sizeof(shray_pair_distance), nullptr, counts}, count,
        op->max_pairs, tallies,
        [&] {
            ShrayQueryScene q;
            int height = 0;
            return enter_walkable_scene(scene, &q, &height);
        },
        [&](void *d_triangles, void *d_out, int32_t *, int32_t *d_counts, DeviceCounters *shards) {
            return clearance_device(scene, op, self, (const shray_triangle *)d_triangles, first, count, (shray_pair_distance *)d_out, d_counts,
                                    nullptr, shards);
        });
}

}   // namespace

static_assert(sizeof(shray_clearance_params) == 16, "shray_clearance_params is 16 bytes");
static_assert(sizeof(shray_pair_distance) == 48 && sizeof(shray_triangle) == 48, "the triangle-distance query's records");

extern "C" {

void shray_clearance_params_init(shray_clearance_params *op)
{
    if (!op)
        return;
    op->struct_size = sizeof(shray_clearance_params);
    op->max_pairs = 1;
    op->flags = 0;
    op->max_dist2 = INFINITY;
}

int shray_clearance_triangles_device(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *d_triangles,
                                     int64_t count, shray_pair_distance *d_out, int32_t *d_counts, void *hip_stream)
{
    return clearance_device(scene, op, false, d_triangles, 0, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_clearance_triangles(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *triangles, int64_t count,
                              shray_pair_distance *out, int32_t *counts)
{
    return clearance_host(scene, op, false, triangles, 0, count, out, counts, nullptr);
}

int shray_clearance_triangles_counters(shray_scene *scene, const shray_clearance_params *op, const shray_triangle *triangles,
                                       int64_t count, shray_pair_distance *out, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : clearance_host(scene, op, false, triangles, 0, count, out, counts, counters);
}

int shray_clearance_self_device(shray_scene *scene, const shray_clearance_params *op, int64_t first, int64_t count,
                                shray_pair_distance *d_out, int32_t *d_counts, void *hip_stream)
{
    return clearance_device(scene, op, true, nullptr, first, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_clearance_self(shray_scene *scene, const shray_clearance_params *op, int64_t first, int64_t count, shray_pair_distance *out,
                         int32_t *counts)
{
    return clearance_host(scene, op, true, nullptr, first, count, out, counts, nullptr);
}

}   // extern "C"
