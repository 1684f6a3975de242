// intersect.hip -- include/shader_ray_intersect.h: every triangle of a resident scene that intersects each query triangle,
// counted, the K smallest indices kept in order.  The queries are caller-supplied triangles or the
// scene's own.
//
// One lane per query in one-wave workgroups.  The walk is overlap/overlap.hip's: the 32-byte records of octant copy 7 of the
// packed tree (point/packed_walk.h), a level-major LDS column of node names, one entry per edge of the tree's height, both
// children loaded and tested, a popped node not retested.  A node is entered iff its box overlaps the query's vertex box on
// all three axes: six comparisons of stored floats, exact because stage 0 of the header's test is the same comparison on the
// triangle's own vertex box and a node's box is the min/max of the vertices below it.  That is the only cull.  Every triangle
// of a visited leaf takes the header's test, in index order.  The set does not depend on the visit order (the header).
//
// Where a query's nine floats come from (the item array, or the scene's positions for the self form) and whether triangles
// that share a corner are skipped are wave-uniform runtime branches on the launch's arguments, not template parameters: the
// instances stay the twelve of overlap.hip (five slot counts and ANY, each with and without the work counters).
//
// The K smallest indices are kept by sorted insertion: in registers for K <= 8 (instances for 1, 2, 4 and 8 slots; every
// index is a compile-time constant, so there is no scratch), else in the query's own K output slots.  The per-pair test is
// point/triangle_pair_test.h's and the cull point/triangle_box_test.h's, which the instanced form compiles too.
// This library is built apart from libshray_hip.so, so the renderer's and the other clients' code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "params_check.h"
#include "shader_ray_intersect.h"
#include "triangle_pair_test.h"

using namespace shray;

namespace {

constexpr uint32_t kEmpty = 0xffffffffu;   // SHRAY_HIT_MISS as an unsigned index: after every triangle

struct IntersectWork {
    const float4 *triangles;   // three per query: (a, pad), (b, pad), (c, pad); nullptr: the scene's own triangles
    int32_t *out;              // k per query; not touched when k == 0
    int32_t *counts;           // one per query, or nullptr
    uint64_t count;
    uint64_t first;            // this launch's first query
    uint64_t self_first;       // the scene triangle of query 0 (the self form)
    int32_t k;                 // indices per query
    uint32_t skip_shared;      // SHRAY_INTERSECT_SKIP_SHARED is set
    DeviceCounters *counters;
};

// One lane per query.  SLOTS: the register slots of the K smallest indices (k <= SLOTS), kSlotsInMemory: they live in the
// query's output slots (any k, also 0).  ANY: stop at the first member (k is 0).  COUNT: the work counters.
template <int SLOTS, bool ANY, bool COUNT>
__global__ void __launch_bounds__(kBlock) intersect_kernel(SceneView sc, IntersectWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t intersect_stack[];
    uint32_t *column = intersect_stack + threadIdx.x;   // level-major: a wave's accesses are consecutive
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
    const int k = w.k;
    int32_t *slots = w.out + index * (uint64_t)k;   // this query's own (dereferenced only when live and k > 0)

    constexpr int R = SLOTS > 0 ? SLOTS : 1;
    uint32_t held[R];   // ascending; (plain scalars: every index below is a constant once unrolled)
#pragma unroll
    for (int i = 0; i < R; i++)
        held[i] = kEmpty;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            slots[i] = SHRAY_HIT_MISS;
    int n = 0;
    unsigned int nodes = 0, leaves = 0, tests = 0;

    if (walk) {
        const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
        Record cur = load_record(copy, sc.packed_root);
        nodes++;
        int sp = 0;
        bool go = boxes_overlap(cur.box, q.lo, q.hi);
        while (go) {
            if (cur.b & kLeafFlag) {
                leaves++;
                const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
                for (uint32_t t = first; t < first + in_leaf; t++) {
                    tests++;
                    if (!triangle_intersects(q, skip_shared, sc.positions + 9ull * t))
                        continue;
                    n++;
                    if (ANY)
                        break;
                    if (SLOTS != kSlotsInMemory) {
                        // the index sinks to where it sorts, the largest falls off
                        uint32_t carry = t;
#pragma unroll
                        for (int i = 0; i < R; i++) {
                            const uint32_t low = carry < held[i] ? carry : held[i];
                            carry = carry < held[i] ? held[i] : carry;
                            held[i] = low;
                        }
                    } else if (k > 0 && t < (uint32_t)slots[k - 1]) {
                        int i = k - 1;
                        while (i > 0) {
                            const int32_t s = slots[i - 1];
                            if (!(t < (uint32_t)s))
                                break;
                            slots[i] = s;
                            i--;
                        }
                        slots[i] = (int32_t)t;
                    }
                }
                if (ANY && n > 0)
                    break;
            } else {
                const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                const Record r0 = load_record(copy, n0), r1 = load_record(copy, n1);
                nodes += 2;
                const bool in0 = boxes_overlap(r0.box, q.lo, q.hi), in1 = boxes_overlap(r1.box, q.lo, q.hi);
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
    if (live) {
        if (SLOTS != kSlotsInMemory) {
#pragma unroll
            for (int i = 0; i < R; i++)
                if (i < k)
                    slots[i] = (int32_t)held[i];
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

constexpr Nouns kNouns = {"triangle", "triangles", "scene", "out", "max_triangles", "triangle-intersection query"};
constexpr uint32_t kKnownFlags = SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_SHARED;

// the checks every form makes before it touches a scene or a device; the self form's `triangles` is its scene (it has no
// item array) and its `first` the first of the scene's triangles, 0 for the item forms
int check_query(shray_scene *scene, const shray_intersect_params *op, const void *triangles, int64_t first, int64_t count, const void *out,
                const void *counts)
{
    const int rc = check_params(op, kKnownFlags);
    if (rc)
        return rc;
    return check_first_k(kNouns, scene, triangles, count, op->max_triangles, out, counts, [&] {
        if (first < 0)
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative first triangle %lld", (long long)first);
        return check_any(op, counts);
    });
}

int check_alignment(const void *triangles, const void *out, const void *counts)
{
    if (!aligned(triangles, 16) || (out && !aligned(out, 4)) || (counts && !aligned(counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the triangles must be 16-byte aligned, the indices and the counts 4-byte aligned");
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

// (this walk has no form that prunes: the choice is the work counters alone)
template <int SLOTS>
void launch_form(dim3 grid, size_t lds, hipStream_t stream, const SceneView &view, const IntersectWork &w)
{
    if (w.counters)
        hipLaunchKernelGGL((intersect_kernel<SLOTS, false, true>), grid, dim3(kBlock), lds, stream, view, w);
    else
        hipLaunchKernelGGL((intersect_kernel<SLOTS, false, false>), grid, dim3(kBlock), lds, stream, view, w);
}

// The device form of both kinds of query: d_triangles, or with self the scene's own triangles [first, first + count).
int intersect_device(shray_scene *scene, const shray_intersect_params *op, bool self, const shray_triangle *d_triangles, int64_t first,
                     int64_t count, int32_t *d_out, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(scene, op, self ? (const void *)scene : d_triangles, first, count, d_out, d_counts);
    if (rc)
        return rc;
    const int k = op->max_triangles;
    const bool any = (op->flags & SHRAY_INTERSECT_ANY) != 0;
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
    IntersectWork w{self ? nullptr : (const float4 *)d_triangles, k > 0 ? d_out : nullptr, d_counts, (uint64_t)count, 0, (uint64_t)first, k,
                    (op->flags & SHRAY_INTERSECT_SKIP_SHARED) ? 1u : 0u, d_counters};
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint32_t);
    return first_k_launches(kNouns, w, count, [&](dim3 grid) {
        if (any && d_counters)
            hipLaunchKernelGGL((intersect_kernel<kSlotsInMemory, true, true>), grid, dim3(kBlock), lds, stream, q.view, w);
        else if (any)
            hipLaunchKernelGGL((intersect_kernel<kSlotsInMemory, true, false>), grid, dim3(kBlock), lds, stream, q.view, w);
        else
            with_slots(k, [&](auto slots) { launch_form<decltype(slots)::value>(grid, lds, stream, q.view, w); });
    });
}

// the blocking forms: the triangles to the device (none for the self form), the query on the null stream, the indices,
// counts (and tallies) back
int intersect_host(shray_scene *scene, const shray_intersect_params *op, bool self, const shray_triangle *triangles, int64_t first,
                   int64_t count, int32_t *out, int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(scene, op, self ? (const void *)scene : triangles, first, count, out, counts))
        return rc;
    if (const int rc = check_alignment(self ? nullptr : triangles, out, counts))
        return rc;
    if (self)
        if (const int rc = check_self_range(scene, first, count))
            return rc;
    static const float no_items[4] = {};
    return first_k_blocking(
        {self ? (const void *)no_items : triangles, self ? 0 : sizeof(shray_triangle), out, sizeof(int32_t), nullptr, counts}, count,
        op->max_triangles, tallies,
        [&] {
            ShrayQueryScene q;
            int height = 0;
            return enter_walkable_scene(scene, &q, &height);
        },
        [&](void *d_triangles, void *d_out, int32_t *, int32_t *d_counts, DeviceCounters *shards) {
            return intersect_device(scene, op, self, (const shray_triangle *)d_triangles, first, count, (int32_t *)d_out, d_counts, nullptr,
                                    shards);
        });
}

}   // namespace

static_assert(sizeof(shray_intersect_params) == 16, "shray_intersect_params is 16 bytes");
static_assert(sizeof(shray_triangle) == 48, "shray_triangle is 48 bytes");

extern "C" {

void shray_intersect_params_init(shray_intersect_params *op)
{
    if (!op)
        return;
    op->struct_size = sizeof(shray_intersect_params);
    op->max_triangles = 8;
    op->flags = 0;
    op->reserved = 0;
}

int shray_intersect_triangles_device(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *d_triangles,
                                     int64_t count, int32_t *d_out, int32_t *d_counts, void *hip_stream)
{
    return intersect_device(scene, op, false, d_triangles, 0, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_intersect_triangles(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *triangles, int64_t count,
                              int32_t *out, int32_t *counts)
{
    return intersect_host(scene, op, false, triangles, 0, count, out, counts, nullptr);
}

int shray_intersect_triangles_counters(shray_scene *scene, const shray_intersect_params *op, const shray_triangle *triangles,
                                       int64_t count, int32_t *out, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : intersect_host(scene, op, false, triangles, 0, count, out, counts, counters);
}

int shray_intersect_self_device(shray_scene *scene, const shray_intersect_params *op, int64_t first, int64_t count, int32_t *d_out,
                                int32_t *d_counts, void *hip_stream)
{
    return intersect_device(scene, op, true, nullptr, first, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_intersect_self(shray_scene *scene, const shray_intersect_params *op, int64_t first, int64_t count, int32_t *out, int32_t *counts)
{
    return intersect_host(scene, op, true, nullptr, first, count, out, counts, nullptr);
}

}   // extern "C"
