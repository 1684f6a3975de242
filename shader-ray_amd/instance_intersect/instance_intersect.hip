// instance_intersect.hip -- include/shader_ray_instance_intersect.h: every triangle of every instance of a set of placed
// scenes that intersects each query triangle, counted, the K smallest (instance, triangle) pairs kept in order (DESIGN
// section 24).  The queries are caller-supplied world triangles or the triangles of one instance under its own map.
//
// One lane per query in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level): a lane enters a node unless an axis separates the node's stored box from its query's vertex box, and near
// zero an axis may not separate (instance/image_box.h's kGuard).  At a leaf the instance is
// wave-uniform: its forward map's three rows and the member's SceneView come in by scalar loads, and the entering lanes run the
// walk of intersect/intersect.hip over that member's packed tree with every box replaced by its image box under the map and
// every triangle's corners mapped before the per-pair test.  A lane's K smallest carry from one instance into the next under
// the key (instance, triangle).
//
// Where a query's nine floats come from (the item array, or instance q's scene under instance q's map), whether triangles that
// share a corner are skipped and whether the query's own instance is skipped are wave-uniform runtime branches on the launch's
// arguments, not template parameters: the instances stay instance_overlap.hip's.
//
// The K smallest are kept as instance_overlap.hip keeps them: in registers for K <= 8 (one 64-bit key a slot, every index a
// compile-time constant, no scratch), else the triangles in the query's own K output slots and the instances in the instance
// buffer beside them (instance/held_pairs.h's Held).  The image boxes, the corner mapping and the guard are
// instance/image_box.h's, the per-pair test point/triangle_pair_test.h's: this library compiles the code that
// libshray_instance_overlap.so and libshray_intersect.so compile.  It is built apart from libshray_hip.so and
// libshray_instance.so, so their code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "enter_set.h"
#include "first_k_query.h"
#include "held_pairs.h"
#include "image_box.h"
#include "packed_walk.h"
#include "params_check.h"
#include "shader_ray_instance_intersect.h"
#include "top_level.h"
#include "trace_common.h"
#include "triangle_pair_test.h"

using namespace shray;

namespace {

struct SetIntersectWork {
    const float4 *triangles;   // three per query: (a, pad), (b, pad), (c, pad), world space; nullptr: the instance form
    int32_t *out;              // k per query: triangles; not touched when k == 0
    int32_t *instances;        // k per query, or nullptr (never nullptr for the form that keeps its K smallest in memory, k > 0)
    int32_t *counts;           // one per query, or nullptr
    uint64_t count;
    uint64_t first;            // this launch's first query
    uint64_t own_first;        // the instance form: the scene triangle of query 0
    int32_t own;               // the instance form: the instance the queries are of
    int32_t k;                 // pairs per query
    int32_t stack_levels;      // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    uint32_t skip_shared;      // SHRAY_INTERSECT_SKIP_SHARED is set
    uint32_t skip_own;         // SHRAY_INTERSECT_SKIP_OWN_INSTANCE is set
    DeviceCounters *counters;
};

// One lane's walk of instance `inst`: intersect.hip's loop over the member's packed tree, on image boxes and mapped corners.
template <int SLOTS, bool ANY>
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], int inst, const Query &q, bool skip_shared,
                                              uint32_t *column, Held<SLOTS> &held, int &n, unsigned int &nodes, unsigned int &leaves,
                                              unsigned int &tests)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    Record cur = load_record(copy, sc.packed_root);
    nodes++;
    int sp = 0;
    bool go = image_overlaps(m, cur.box, q.lo, q.hi);
    while (go) {
        if (cur.b & kLeafFlag) {
            leaves++;
            const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
            for (uint32_t t = first; t < first + in_leaf; t++) {
                tests++;
                float c9[9];
                mapped_corners(m, sc.positions, t, c9);
                if (!triangle_intersects(q, skip_shared, c9))
                    continue;
                n++;
                if (ANY)
                    break;
                held.insert(inst, t);
            }
            if (ANY && n > 0)
                break;
        } else {
            const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
            const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
            nodes += 2;
            const bool in0 = image_overlaps(m, r0.box, q.lo, q.hi), in1 = image_overlaps(m, r1.box, q.lo, q.hi);
            if (in0 || in1) {
                if (in0 && in1) {
                    column[(size_t)sp * kBlock] = n1;
                    sp++;
                }
                cur = in0 ? r0 : r1;
                continue;
            }
        }
        // pop: the stack holds at most one entry per level of the current path, each already tested against the box
        go = sp > 0;
        if (go) {
            sp--;
            cur = load_record(copy, column[(size_t)sp * kBlock]);
        }
    }
}

// One lane per query.  SLOTS: the register slots of the K smallest pairs (k <= SLOTS), kSlotsInMemory: they live in the
// query's output slots (any k, also 0).  PRUNE: a lane that holds K pairs skips an instance above all of them.  COUNT: the
// work counters.  ANY: a lane stops at its first member (k is 0).  The pointers are __restrict__ so that a leaf's record, its
// map and its SceneView, and in the instance form the queries' own, come in by scalar loads.
template <int SLOTS, bool PRUNE, bool COUNT, bool ANY>
__global__ void __launch_bounds__(kBlock) instance_intersect_kernel(SetIntersectWork w, const TopNode *__restrict__ nodes,
                                                                    const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                                    const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t intersect_stack[];
    uint32_t *column = intersect_stack + threadIdx.x;                        // level-major: a wave's accesses are consecutive
    uint32_t *top = intersect_stack + (size_t)kBlock * w.stack_levels;      // the wave's top-level stack
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
    bool walk = live;
    float f0[3], f1[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        walk = walk && __builtin_isfinite(q.p[0][j]) && __builtin_isfinite(q.p[1][j]) && __builtin_isfinite(q.p[2][j]);
        q.lo[j] = min3(q.p[0][j], q.p[1][j], q.p[2][j]);
        q.hi[j] = max3(q.p[0][j], q.p[1][j], q.p[2][j]);
        const float q0 = q.p[0][j] - q.p[0][j];
        q.q1[j] = q.p[1][j] - q.p[0][j];
        q.q2[j] = q.p[2][j] - q.p[0][j];
        f0[j] = q.q1[j] - q0;
        f1[j] = q.q2[j] - q.q1[j];
    }
    cross(q.nq, f0, f1);
    walk = walk && !all_zero(q.nq);   // a degenerate query is not walked
    const bool skip_shared = w.skip_shared != 0;
    const int skipped = w.skip_own ? w.own : -1;   // the instance whose pairs are no members (no instance is -1)
    const int k = w.k;

    Held<SLOTS> held;
    held.k = k;
    held.slots = w.out + index * (uint64_t)k;   // this query's own (dereferenced only when live and k > 0)
    held.slot_inst = w.instances + index * (uint64_t)k;
#pragma unroll
    for (int i = 0; i < Held<SLOTS>::R; i++)
        held.key[i] = kEmptyKey;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            held.slots[i] = SHRAY_HIT_MISS, held.slot_inst[i] = -1;
    int n = 0;
    unsigned int visited = 0, leaves = 0, tests = 0, walks = 0;

    if (__builtin_amdgcn_ballot_w64(walk)) {
        walk_top_level(
            nodes, top,
            // No axis separates the stored box from the query's vertex box, near zero by the guard's leave.  The root is not tested.
            [&](uint32_t node, const float4 &a, const float4 &b) {
                return walk && !(ANY && n > 0) && (node == 0u || stored_overlaps(a, b, q.lo, q.hi));
            },
            // the lower child first (the walk's order affects its speed only)
            [&](uint32_t, uint32_t, unsigned long long) { return true; },
            [&](int inst, bool enters) {
                if (inst == skipped)   // (wave-uniform)
                    return;
                const float4 *row = maps + 3u * (uint32_t)inst;
                const float4 m[3] = {row[0], row[1], row[2]};
                const SceneView &sc = leaf_view(records, views, inst);
                if (enters && !(PRUNE && held.full_below(inst))) {
                    walks++;
                    instance_walk<SLOTS, ANY>(sc, m, inst, q, skip_shared, column, held, n, visited, leaves, tests);
                }
            });
    }
    if (live) {
        if (SLOTS != kSlotsInMemory) {
#pragma unroll
            for (int i = 0; i < Held<SLOTS>::R; i++)
                if (i < k) {
                    const bool empty = held.key[i] == kEmptyKey;
                    held.slots[i] = empty ? SHRAY_HIT_MISS : (int32_t)(uint32_t)held.key[i];
                    if (w.instances)
                        held.slot_inst[i] = empty ? -1 : (int32_t)(held.key[i] >> 32);
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

constexpr Nouns kNouns = {"triangle", "triangles", "set", "out", "max_triangles", "instanced triangle-intersection query"};
constexpr uint32_t kItemFlags = SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_SHARED;   // only the instance form knows SKIP_OWN_INSTANCE

// where a form's queries come from: the item array, or the triangles [first, first + count) of instance `instance`
struct Source {
    bool own;
    int32_t instance;
    int64_t first;
};

// The checks every form makes before it touches a device.  The instance form's `triangles` is its set (it has no item array).
int check_query(shray_instance_set *set, const shray_intersect_params *op, const Source &src, const void *triangles, int64_t count,
                const void *out, const void *instances, const void *counts)
{
    int rc = check_params(op, kItemFlags | (src.own ? (uint32_t)SHRAY_INTERSECT_SKIP_OWN_INSTANCE : 0u));
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
    if ((rc = check_first_k(kNouns, set, src.own ? (const void *)set : triangles, count, op->max_triangles, out, counts)))
        return rc;
    if ((!src.own && !aligned(triangles, 16)) || !aligned(out, 4) || !aligned(instances, 4) || !aligned(counts, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT,
                    "the triangles must be 16-byte aligned, the indices, the instances and the counts 4-byte aligned");
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

int intersect_device(shray_instance_set *set, const shray_intersect_params *op, const Source &src, const shray_triangle *d_triangles,
                     int64_t count, int32_t *d_out, int32_t *d_instances, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(set, op, src, d_triangles, count, d_out, d_instances, d_counts);
    if (rc || (rc = check_own_range(set, src, count)))
        return rc;
    const int k = op->max_triangles;
    const bool any = (op->flags & SHRAY_INTERSECT_ANY) != 0;
    if (count == 0)
        return SHRAY_OK;
    return walk_set(set, true, k, count, d_instances, stream, [&](const SetWalk &s) {
        SetIntersectWork w{src.own ? nullptr : (const float4 *)d_triangles,
                           k > 0 ? d_out : nullptr,
                           k > 0 ? s.instances : nullptr,
                           d_counts,
                           (uint64_t)count,
                           0,
                           src.own ? (uint64_t)src.first : 0,
                           src.own ? src.instance : -1,
                           k,
                           s.levels,
                           (op->flags & SHRAY_INTERSECT_SKIP_SHARED) ? 1u : 0u,
                           (op->flags & SHRAY_INTERSECT_SKIP_OWN_INSTANCE) ? 1u : 0u,
                           d_counters};
        const size_t lds = s.lds(sizeof(uint32_t));
        return first_k_launches(kNouns, w, count, [&](dim3 grid) {
            if (any && d_counters)
                hipLaunchKernelGGL((instance_intersect_kernel<kSlotsInMemory, false, true, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else if (any)
                hipLaunchKernelGGL((instance_intersect_kernel<kSlotsInMemory, false, false, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else
                with_slots(k, [&](auto slots) {
                    with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                        hipLaunchKernelGGL(
                            (instance_intersect_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value, false>), grid,
                            dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
                    });
                });
        });
    });
}

// the blocking forms: the triangles to the device (none for the instance form), the query on the null stream, the indices,
// instances, counts (and tallies) back
int intersect_host(shray_instance_set *set, const shray_intersect_params *op, const Source &src, const shray_triangle *triangles,
                   int64_t count, int32_t *out, int32_t *instances, int32_t *counts, shray_counters *tallies)
{
    int rc = check_query(set, op, src, triangles, count, out, instances, counts);
    if (rc || (rc = check_own_range(set, src, count)))
        return rc;
    static const float no_items[4] = {};
    return first_k_blocking(
        {src.own ? (const void *)no_items : triangles, src.own ? 0 : sizeof(shray_triangle), out, sizeof(int32_t), instances, counts}, count,
        op->max_triangles, tallies,
        [&] { return enter_set(set); },
        [&](void *d_triangles, void *d_out, int32_t *d_instances, int32_t *d_counts, DeviceCounters *shards) {
            return intersect_device(set, op, src, (const shray_triangle *)d_triangles, count, (int32_t *)d_out, d_instances, d_counts, nullptr,
                                    shards);
        });
}

constexpr Source kItems = {false, -1, 0};

}   // namespace

static_assert(sizeof(shray_intersect_params) == 16, "shray_intersect_params is 16 bytes");
static_assert(sizeof(shray_triangle) == 48, "shray_triangle is 48 bytes");
static_assert((SHRAY_INTERSECT_SKIP_OWN_INSTANCE & (SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_SHARED)) == 0, "a flag bit of its own");

extern "C" {

int shray_intersect_triangles_instances_device(shray_instance_set *set, const shray_intersect_params *op,
                                               const shray_triangle *d_triangles, int64_t count, int32_t *d_out, int32_t *d_instances,
                                               int32_t *d_counts, void *hip_stream)
{
    return intersect_device(set, op, kItems, d_triangles, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_intersect_triangles_instances(shray_instance_set *set, const shray_intersect_params *op, const shray_triangle *triangles,
                                        int64_t count, int32_t *out, int32_t *instances, int32_t *counts)
{
    return intersect_host(set, op, kItems, triangles, count, out, instances, counts, nullptr);
}

int shray_intersect_triangles_instances_counters(shray_instance_set *set, const shray_intersect_params *op,
                                                 const shray_triangle *triangles, int64_t count, int32_t *out, int32_t *instances,
                                                 int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : intersect_host(set, op, kItems, triangles, count, out, instances, counts, counters);
}

int shray_intersect_instance_device(shray_instance_set *set, const shray_intersect_params *op, int32_t instance, int64_t first,
                                    int64_t count, int32_t *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return intersect_device(set, op, Source{true, instance, first}, nullptr, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream,
                            nullptr);
}

int shray_intersect_instance(shray_instance_set *set, const shray_intersect_params *op, int32_t instance, int64_t first, int64_t count,
                             int32_t *out, int32_t *instances, int32_t *counts)
{
    return intersect_host(set, op, Source{true, instance, first}, nullptr, count, out, instances, counts, nullptr);
}

}   // extern "C"
