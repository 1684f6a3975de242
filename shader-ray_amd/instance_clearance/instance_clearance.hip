// instance_clearance.hip -- include/shader_ray_instance_clearance.h: every triangle of every instance of a set of placed scenes
// within a squared distance of each query triangle, counted, the nearest K kept in order with their instances, each with its
// dist2 and a witness on either triangle.  The queries are caller-supplied world triangles or the triangles
// of one instance under its own map.
//
// One lane per query in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level, with the instanced within-radius query's enter predicate and child order, instance_near/instance_near.hip,
// and a box for its point): a lane enters a node unless the squared gap between the node's stored box and its query's vertex
// box is above its reach: max_dist2, or, in the form that is not asked for counts, the K-th smallest dist2 it holds.  At a leaf
// the instance is wave-uniform: its forward map's three rows and the member's SceneView come in by scalar loads, and the
// entering lanes run the walk of clearance/clearance.hip over that member's packed tree with every box replaced by its image
// box under the map and every triangle's corners mapped before the per-pair arithmetic.  A lane's K best carry from one
// instance into the next under the key (dist2, instance, triangle).
//
// The K best are kept as instance_near.hip keeps them: their keys in registers for K <= 8 (three words a slot, every index a
// compile-time constant, no scratch), the winners' records computed again at the end by the same function on the same mapped
// corners (the winners' instances are not wave-uniform, so the map and the positions then come by per-lane loads); for
// larger K the whole records are inserted into the query's own K output slots and the instances into the instance buffer.
// Where a query's nine floats come from (the item array, or instance q's scene under instance q's map), whether triangles that
// share a corner are skipped and whether the query's own instance is skipped are wave-uniform runtime branches on the launch's
// arguments, as in instance_intersect/instance_intersect.hip.
// The image boxes and the corner mapping are instance/image_box.h's, the per-pair arithmetic and the box-to-box bound
// point/triangle_pair_distance.h's: this library compiles the code that libshray_instance_near.so and libshray_clearance.so
// compile.  It is built apart from libshray_hip.so and libshray_instance.so, so their code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "enter_set.h"
#include "first_k_query.h"
#include "image_box.h"
#include "packed_walk.h"
#include "params_check.h"
#include "shader_ray_instance_clearance.h"
#include "top_level.h"
#include "trace_common.h"
#include "triangle_pair_distance.h"

using namespace shray;

namespace {

struct SetClearanceWork {
    const float4 *triangles;   // three per query: (a, pad), (b, pad), (c, pad), world space; nullptr: the instance form
    float4 *out;               // 3 * k per query: (x, dist2), (y, triangle bits), (feature bits, 0, 0, 0); not touched when k == 0
    int32_t *instances;        // k per query, or nullptr (never nullptr for the form that keeps its K best in memory, k > 0)
    int32_t *counts;           // one per query, or nullptr
    uint64_t count;
    uint64_t first;            // this launch's first query
    uint64_t own_first;        // the instance form: the scene triangle of query 0
    int32_t own;               // the instance form: the instance the queries are of
    int32_t k;                 // records per query
    int32_t stack_levels;      // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    uint32_t skip_shared;      // SHRAY_CLEARANCE_SKIP_SHARED is set
    uint32_t skip_own;         // SHRAY_CLEARANCE_SKIP_OWN_INSTANCE is set
    float max_dist2;
    DeviceCounters *counters;
};

// the key of the header: dist2 as a float comparison, then the instance, then the triangle; an empty slot (triangle < 0) is
// after every member
__device__ __forceinline__ bool before(float d, int inst, int tri, float slot_d, int slot_inst, int slot_tri)
{
    return slot_tri < 0 || d < slot_d || (d == slot_d && (inst < slot_inst || (inst == slot_inst && tri < slot_tri)));
}

__device__ __forceinline__ void store_record(float4 *slot, const PairDistance &r, int tri)
{
    slot[0] = make_float4(r.x[0], r.x[1], r.x[2], r.dist2);
    slot[1] = make_float4(r.y[0], r.y[1], r.y[2], __int_as_float(tri));
    slot[2] = make_float4(__int_as_float(r.feature), 0.0f, 0.0f, 0.0f);
}

// the record of the pair (the instance whose map is m, triangle t of its scene): the corners mapped, then the pair arithmetic
__device__ __forceinline__ PairDistance pair_on_mapped(const float4 (&m)[3], const float *positions, uint32_t t, const Query &q)
{
    return with_mapped_corners(m, positions, t, [&](const float *c9) { return pair_distance(q, c9); });
}

// a box's bound: the squared gap between it and the query's vertex box
__device__ __forceinline__ float image_gap2(const float4 (&m)[3], const Query &q, const Box &b)
{
    const Box o = image_box(m, b);
    return box_gap2(q.lo, q.hi, o.lo, o.hi);
}

// A lane's K best.  SLOTS > 0: the keys in registers; kSlotsInMemory: the records in the query's own output slots and
// their instances beside them (any k, also 0).
template <int SLOTS>
struct Held {
    static constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float d[R];   // (plain scalars: every index is a constant once unrolled)
    int inst[R], tri[R];
    float4 *slots;       // in memory: this query's own records and instances (dereferenced only when live and k > 0)
    int32_t *slot_inst;
    int k;

    // the key moves in where it sorts, the rest move down, the last falls off; returns the dist2 of slot k - 1 afterwards
    // when PRUNE (an empty slot holds max_dist2), else `reach` as it was
    template <bool PRUNE>
    __device__ __forceinline__ float insert(const PairDistance &c, int in, int t, float reach)
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
        } else if (k > 0 && before(dist2, in, t, slots[3 * (k - 1)].w, slot_inst[k - 1], __float_as_int(slots[3 * (k - 1) + 1].w))) {
            int i = k - 1;
            while (i > 0) {
                const float4 s0 = slots[3 * (i - 1)], s1 = slots[3 * (i - 1) + 1];
                const float feature = slots[3 * (i - 1) + 2].x;   // (the rest of a record's third word is the reserved zeros)
                const int si = slot_inst[i - 1];
                if (!before(dist2, in, t, s0.w, si, __float_as_int(s1.w)))
                    break;
                // (component by component: a whole-vector copy of a word whose .w alone is read went through scratch)
                slots[3 * i] = make_float4(s0.x, s0.y, s0.z, s0.w), slots[3 * i + 1] = make_float4(s1.x, s1.y, s1.z, s1.w);
                slots[3 * i + 2] = make_float4(feature, 0.0f, 0.0f, 0.0f);
                slot_inst[i] = si;
                i--;
            }
            store_record(slots + 3 * i, c, t);
            slot_inst[i] = in;
            if (PRUNE)
                reach = slots[3 * (k - 1)].w;   // (a miss record holds max_dist2)
        }
        return reach;
    }
};

// One lane's walk of instance `inst`: clearance.hip's loop over the member's packed tree, on image boxes and mapped corners.
template <int SLOTS, bool PRUNE, bool ANY>
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], int inst, const Query &q, bool skip_shared,
                                              float md, uint32_t *column, Held<SLOTS> &held, float &reach, int &n, unsigned int &nodes,
                                              unsigned int &leaves, unsigned int &tests)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    Record cur = load_record(copy, sc.packed_root);
    nodes++;
    int sp = 0;
    bool go = !(image_gap2(m, q, cur.box) > reach);
    while (go) {
        if (cur.b & kLeafFlag) {
            leaves++;
            const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
            for (uint32_t t = first; t < first + in_leaf; t++) {
                const bool member = with_mapped_corners(m, sc.positions, t, [&](const float *c9) {
                    if (skip_shared && shares_corner(q, c9))
                        return false;
                    if (triangle_gap2(q, c9) > reach)   // the pair's dist2 is no less
                        return false;
                    tests++;
                    const PairDistance c = pair_distance(q, c9);
                    if (!(c.dist2 <= md))
                        return false;
                    n++;
                    if (!ANY)
                        reach = held.template insert<PRUNE>(c, inst, (int)t, reach);
                    return true;
                });
                if (ANY && member)
                    break;
            }
            if (ANY && n > 0)
                break;
        } else {
            const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
            const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
            const float lb0 = image_gap2(m, q, r0.box), lb1 = image_gap2(m, q, r1.box);
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
            if (PRUNE && image_gap2(m, q, cur.box) > reach)   // the reach has dropped below it since the push
                continue;
            go = true;
            break;
        }
    }
}

// One lane per query.  SLOTS: the register slots of the K best keys (k <= SLOTS), kSlotsInMemory: the records live in the
// query's output slots (any k, also 0).  PRUNE: skip what cannot reach the nearest k (no count is written).  COUNT: the work
// counters.  ANY: a lane stops at its first member (k is 0).  The pointers are __restrict__ so that a leaf's record, its map
// and its SceneView, and in the instance form the queries' own, come in by scalar loads.
template <int SLOTS, bool PRUNE, bool COUNT, bool ANY>
__global__ void __launch_bounds__(kBlock) instance_clearance_kernel(SetClearanceWork w, const TopNode *__restrict__ nodes,
                                                                    const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                                    const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t clearance_stack[];
    uint32_t *column = clearance_stack + threadIdx.x;                       // level-major: a wave's accesses are consecutive
    uint32_t *top = clearance_stack + (size_t)kBlock * w.stack_levels;      // the wave's top-level stack
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    Query q;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            q.p[i][j] = 0.0f;
    if (w.triangles) {
        if (live) {
            const float4 c0 = w.triangles[3 * index], c1 = w.triangles[3 * index + 1], c2 = w.triangles[3 * index + 2];
            q.p[0][0] = c0.x, q.p[0][1] = c0.y, q.p[0][2] = c0.z;
            q.p[1][0] = c1.x, q.p[1][1] = c1.y, q.p[1][2] = c1.z;
            q.p[2][0] = c2.x, q.p[2][1] = c2.y, q.p[2][2] = c2.z;
        }
    } else {
        // the instance form: w.own is uniform, so its map and its view are scalar loads; the corners are that instance's
        // world corners, by the formula every pair's are mapped with
        const float4 *row = maps + 3u * (uint32_t)w.own;
        const float4 m[3] = {row[0], row[1], row[2]};
        const SceneView &sc = leaf_view(records, views, w.own);
        if (live) {   // (the host checked the range)
            float c9[9];
            mapped_corners(m, sc.positions, w.own_first + index, c9);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    q.p[i][j] = c9[3 * i + j];
        }
    }
    const float md = w.max_dist2;
    const bool walk = make_query(q) && live && md >= 0.0f;   // (a NaN max_dist2 fails the comparison)
    const bool skip_shared = w.skip_shared != 0;
    const int skipped = w.skip_own ? w.own : -1;   // the instance whose pairs are no members (no instance is -1)
    const int k = w.k;
    const float4 miss0 = make_float4(0.0f, 0.0f, 0.0f, md);
    const float4 miss1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS));
    const float4 miss2 = make_float4(__int_as_float(-1), 0.0f, 0.0f, 0.0f);

    Held<SLOTS> held;
    held.k = k;
    held.slots = w.out + 3ull * (index * (uint64_t)k);        // this query's own (dereferenced only when live and k > 0)
    held.slot_inst = w.instances + index * (uint64_t)k;
#pragma unroll
    for (int i = 0; i < Held<SLOTS>::R; i++)
        held.d[i] = md, held.inst[i] = -1, held.tri[i] = SHRAY_HIT_MISS;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            held.slots[3 * i] = miss0, held.slots[3 * i + 1] = miss1, held.slots[3 * i + 2] = miss2, held.slot_inst[i] = -1;
    // what a bound must not exceed: max_dist2, or (PRUNE) the k-th smallest dist2 held, max_dist2 while fewer are held
    float reach = md;
    int n = 0;
    unsigned int visited = 0, leaves = 0, tests = 0, walks = 0;

    if (__builtin_amdgcn_ballot_w64(walk)) {
        walk_top_level(
            nodes, top,
            // The bound of the stored box is never above a pair's dist2 below it; a bound that equals the
            // reach enters (a lower instance wins a tie there).  The root is not tested.
            [&](uint32_t node, const float4 &a, const float4 &b) {
                const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
                return walk && !(ANY && n > 0) && (node == 0u || !(box_gap2(q.lo, q.hi, lo, hi) > reach));
            },
            // the nearer child first by the first entering lane's bounds (the walk's order affects its speed only)
            [&](uint32_t, uint32_t left, unsigned long long entering) {
                const float4 la = reinterpret_cast<const float4 *>(nodes)[2u * left], lb = reinterpret_cast<const float4 *>(nodes)[2u * left + 1u];
                const float4 ra = reinterpret_cast<const float4 *>(nodes)[2u * left + 2u], rb = reinterpret_cast<const float4 *>(nodes)[2u * left + 3u];
                const float llo[3] = {la.x, la.y, la.z}, lhi[3] = {lb.x, lb.y, lb.z}, rlo[3] = {ra.x, ra.y, ra.z}, rhi[3] = {rb.x, rb.y, rb.z};
                const int mine = box_gap2(q.lo, q.hi, rlo, rhi) < box_gap2(q.lo, q.hi, llo, lhi) ? 1 : 0;
                return __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(entering)) == 0;
            },
            [&](int inst, bool enters) {
                if (inst == skipped)   // (wave-uniform)
                    return;
                const float4 *row = maps + 3u * (uint32_t)inst;
                const float4 m[3] = {row[0], row[1], row[2]};
                const SceneView &sc = leaf_view(records, views, inst);
                if (enters) {
                    walks++;
                    instance_walk<SLOTS, PRUNE, ANY>(sc, m, inst, q, skip_shared, md, column, held, reach, n, visited, leaves, tests);
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
                if (tri >= 0) {
                    const float4 *row = maps + 3u * (uint32_t)inst;
                    const float4 m[3] = {row[0], row[1], row[2]};
                    store_record(held.slots + 3 * i, pair_on_mapped(m, leaf_view(records, views, inst).positions, (uint32_t)tri, q), tri);
                } else {
                    held.slots[3 * i] = miss0, held.slots[3 * i + 1] = miss1, held.slots[3 * i + 2] = miss2;
                }
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

constexpr Nouns kNouns = {"triangle", "triangles", "set", "out", "max_pairs", "instanced triangle-distance query"};
constexpr uint32_t kItemFlags = SHRAY_CLEARANCE_ANY | SHRAY_CLEARANCE_SKIP_SHARED;   // only the instance form knows SKIP_OWN_INSTANCE

// where a form's queries come from: the item array, or the triangles [first, first + count) of instance `instance`
struct Source {
    bool own;
    int32_t instance;
    int64_t first;
};

// The checks every form makes before it touches a device.  The instance form's `triangles` is its set (it has no item array).
int check_query(shray_instance_set *set, const shray_clearance_params *op, const Source &src, const void *triangles, int64_t count,
                const void *out, const void *instances, const void *counts)
{
    int rc = check_params(op, kItemFlags | (src.own ? (uint32_t)SHRAY_CLEARANCE_SKIP_OWN_INSTANCE : 0u));
    if (rc || (rc = check_any(op, counts)))
        return rc;
    if (src.own) {
        if (src.first < 0)
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative first triangle %lld", (long long)src.first);
        ShrayInstanceSetDevice d;
        if (set && (rc = shrayi_instance_set_device_arrays(set, &d)))
            return rc;
        if (set && (src.instance < 0 || src.instance >= d.count))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %d is not among the set's %d", src.instance, d.count);
    }
    if ((rc = check_first_k(kNouns, set, src.own ? (const void *)set : triangles, count, op->max_pairs, out, counts)))
        return rc;
    if ((!src.own && !aligned(triangles, 16)) || (op->max_pairs > 0 && !aligned(out, 16)) || !aligned(instances, 4) || !aligned(counts, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT,
                    "the triangles and the records must be 16-byte aligned, the instances and the counts 4-byte aligned");
    return SHRAY_OK;
}

// the instance form's range against its instance's scene's triangle count, read on the host
int check_own_range(shray_instance_set *set, const Source &src, int64_t count)
{
    if (!src.own)
        return SHRAY_OK;
    shray_scene *scene = nullptr;
    ShrayQueryScene q;
    int rc = shrayi_instance_set_member_scene(set, src.instance, &scene);
    if (rc || (rc = shrayi_scene_query_view(scene, &q)))
        return rc;
    if ((uint64_t)src.first + (uint64_t)count > q.view.triangle_count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "triangles %lld .. %lld are not all among the %u of instance %d's scene", (long long)src.first,
                    (long long)src.first + (long long)count, q.view.triangle_count, src.instance);
    return SHRAY_OK;
}

int clearance_device(shray_instance_set *set, const shray_clearance_params *op, const Source &src, const shray_triangle *d_triangles,
                     int64_t count, shray_pair_distance *d_out, int32_t *d_instances, int32_t *d_counts, hipStream_t stream,
                     DeviceCounters *d_counters)
{
    int rc = check_query(set, op, src, d_triangles, count, d_out, d_instances, d_counts);
    if (rc || (rc = check_own_range(set, src, count)))
        return rc;
    const int k = op->max_pairs;
    const bool any = (op->flags & SHRAY_CLEARANCE_ANY) != 0;
    if (count == 0)
        return SHRAY_OK;
    return walk_set(set, true, k, count, d_instances, stream, [&](const SetWalk &s) {
        SetClearanceWork w{src.own ? nullptr : (const float4 *)d_triangles,
                           k > 0 ? (float4 *)d_out : nullptr,
                           k > 0 ? s.instances : nullptr,
                           d_counts,
                           (uint64_t)count,
                           0,
                           src.own ? (uint64_t)src.first : 0,
                           src.own ? src.instance : -1,
                           k,
                           s.levels,
                           (op->flags & SHRAY_CLEARANCE_SKIP_SHARED) ? 1u : 0u,
                           (op->flags & SHRAY_CLEARANCE_SKIP_OWN_INSTANCE) ? 1u : 0u,
                           op->max_dist2,
                           d_counters};
        const size_t lds = s.lds(sizeof(uint32_t));
        return first_k_launches(kNouns, w, count, [&](dim3 grid) {
            if (any && d_counters)
                hipLaunchKernelGGL((instance_clearance_kernel<kSlotsInMemory, false, true, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else if (any)
                hipLaunchKernelGGL((instance_clearance_kernel<kSlotsInMemory, false, false, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else
                with_slots(k, [&](auto slots) {
                    with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                        hipLaunchKernelGGL(
                            (instance_clearance_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value, false>), grid,
                            dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
                    });
                });
        });
    });
}

// the blocking forms: the triangles to the device (none for the instance form), the query on the null stream, the records,
// instances, counts (and tallies) back
int clearance_host(shray_instance_set *set, const shray_clearance_params *op, const Source &src, const shray_triangle *triangles,
                   int64_t count, shray_pair_distance *out, int32_t *instances, int32_t *counts, shray_counters *tallies)
{
    int rc = check_query(set, op, src, triangles, count, out, instances, counts);
    if (rc || (rc = check_own_range(set, src, count)))
        return rc;
    static const float no_items[4] = {};
    return first_k_blocking(
        {src.own ? (const void *)no_items : triangles, src.own ? 0 : sizeof(shray_triangle), out, sizeof(shray_pair_distance), instances, counts},
        count, op->max_pairs, tallies, [&] { return enter_set(set); },
        [&](void *d_triangles, void *d_out, int32_t *d_instances, int32_t *d_counts, DeviceCounters *shards) {
            return clearance_device(set, op, src, (const shray_triangle *)d_triangles, count, (shray_pair_distance *)d_out, d_instances,
                                    d_counts, nullptr, shards);
        });
}

constexpr Source kItems = {false, -1, 0};

}   // namespace

static_assert(sizeof(shray_clearance_params) == 16, "shray_clearance_params is 16 bytes");
static_assert(sizeof(shray_pair_distance) == 48 && sizeof(shray_triangle) == 48, "the triangle-distance query's records");
static_assert((SHRAY_CLEARANCE_SKIP_OWN_INSTANCE & (SHRAY_CLEARANCE_ANY | SHRAY_CLEARANCE_SKIP_SHARED)) == 0, "a flag bit of its own");

extern "C" {

int shray_clearance_triangles_instances_device(shray_instance_set *set, const shray_clearance_params *op,
                                               const shray_triangle *d_triangles, int64_t count, shray_pair_distance *d_out,
                                               int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return clearance_device(set, op, kItems, d_triangles, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_clearance_triangles_instances(shray_instance_set *set, const shray_clearance_params *op, const shray_triangle *triangles,
                                        int64_t count, shray_pair_distance *out, int32_t *instances, int32_t *counts)
{
    return clearance_host(set, op, kItems, triangles, count, out, instances, counts, nullptr);
}

int shray_clearance_triangles_instances_counters(shray_instance_set *set, const shray_clearance_params *op,
                                                 const shray_triangle *triangles, int64_t count, shray_pair_distance *out,
                                                 int32_t *instances, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : clearance_host(set, op, kItems, triangles, count, out, instances, counts, counters);
}

int shray_clearance_instance_device(shray_instance_set *set, const shray_clearance_params *op, int32_t instance, int64_t first,
                                    int64_t count, shray_pair_distance *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return clearance_device(set, op, Source{true, instance, first}, nullptr, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream,
                            nullptr);
}

int shray_clearance_instance(shray_instance_set *set, const shray_clearance_params *op, int32_t instance, int64_t first, int64_t count,
                             shray_pair_distance *out, int32_t *instances, int32_t *counts)
{
    return clearance_host(set, op, Source{true, instance, first}, nullptr, count, out, instances, counts, nullptr);
}

}   // extern "C"
