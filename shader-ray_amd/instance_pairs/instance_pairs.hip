// instance_pairs.hip -- include/shader_ray_instance_pairs.h: the collision matrix of a set of placed scenes.  Per ordered pair
// of instances (a, b), the number of pairs (triangle of a, triangle of b) that instance_intersect/'s per-pair test accepts and
// the smallest of them.
//
// The unit of output is a cell, not a query: waves of different workgroups add to the same cell, so a cell is only ever
// touched by agent-scope atomics (a sum, a minimum, or an OR of 1), whose result does not depend on the order of the waves.
//
// One lane per query triangle in one-wave workgroups, and every workgroup belongs to one instance: an instance's triangles are
// padded to a multiple of 64 lanes, and a workgroup finds its instance by a binary search in the prefix sums of the rows'
// workgroup counts (a function of the members' triangle counts only, made on the host).  So the query's instance, its map and
// its SceneView are wave-uniform and come in by scalar loads, as in instance_intersect.hip's instance form, whose query set-up
// this is.  The wave walks the set's top level (instance/top_level.h) with that kernel's predicate; at a leaf the instance b is
// wave-uniform, the entering lanes run instance_intersect.hip's walk of b's packed tree on image boxes and mapped corners
// (restated below without the held pairs: factoring it out of that file would have to leave its code object unchanged), each
// keeping its member count for b and its smallest triangle of b; back at the wave-uniform point the wave reduces them to one
// sum and one smallest key (ta << 32 | tb), and one lane issues at most one atomic add and one atomic min on cell (a, b).
//
// The two skips read a cell with a relaxed agent-scope atomic load.  A cell moves one way only (0 -> 1, a key downward) and
// every value it holds is a member's, so a skip taken on a stale or a fresh read never removes the final value.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "client_internal.h"
#include "enter_set.h"
#include "image_box.h"
#include "packed_walk.h"
#include "shader_ray_instance_pairs.h"
#include "top_level.h"
#include "trace_common.h"
#include "triangle_pair_test.h"

using namespace shray;

namespace {

enum Mode { kAny = 0, kFirstOnly = 1, kCounts = 2 };

constexpr uint32_t kNoTriangle = 0xffffffffu;
constexpr unsigned long long kNone = ~0ull;   // SHRAY_PAIRS_NONE

struct PairsWork {
    unsigned long long *first;    // rows * n keys, or nullptr
    unsigned long long *counts;   // rows * n int64 (never negative: added to as unsigned), or nullptr
    const uint32_t *table;        // rows + 1: the first workgroup of every row, then the grid
    int32_t first_row, rows, n;
    int32_t stack_levels;         // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    uint32_t skip_shared;         // SHRAY_PAIRS_SKIP_SHARED is set
    uint32_t upper;               // SHRAY_PAIRS_UPPER is set
    DeviceCounters *counters;
};

__device__ __forceinline__ unsigned long long cell_now(const unsigned long long *cell)
{
    return __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(x, off);
        x = y < x ? y : x;
    }
    return x;
}

// One lane's walk of instance b: instance_intersect.hip's loop over the member's packed tree, on image boxes and mapped
// corners.  `members` counts the lane's pairs with b, `least` is the smallest of their triangles.
template <bool ANY>
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], const Query &q, bool skip_shared, uint32_t *column,
                                              uint32_t &members, uint32_t &least, unsigned int &nodes, unsigned int &leaves,
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
                members++;
                if (ANY)
                    break;
                least = t < least ? t : least;
            }
            if (ANY && members > 0)
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

// One lane per query triangle, one instance per workgroup.  MODE: what a cell receives (kAny: an OR of 1 into counts;
// kFirstOnly: a minimum into first; kCounts: a sum into counts and, unless first is null, a minimum into first).  COUNT: the
// work counters, and no skip by what a cell holds.  The pointers are __restrict__ so that a leaf's record, its map and its
// SceneView, and the queries' own, come in by scalar loads.
template <int MODE, bool COUNT>
__global__ void __launch_bounds__(kBlock) instance_pairs_kernel(PairsWork w, const TopNode *__restrict__ nodes,
                                                                const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                                const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t pairs_stack[];
    uint32_t *column = pairs_stack + threadIdx.x;                       // level-major: a wave's accesses are consecutive
    uint32_t *top = pairs_stack + (size_t)kBlock * w.stack_levels;     // the wave's top-level stack

    // the row of this workgroup: the last one whose first workgroup is not above it (rows without triangles have none)
    const uint32_t group = blockIdx.x;
    int lo = 0, hi = w.rows;   // table[lo] <= group < table[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (w.table[mid] <= group)
            lo = mid;
        else
            hi = mid;
    }
    const int row = lo;
    const int own = w.first_row + row;
    const uint32_t ta = (group - w.table[row]) * (uint32_t)kBlock + threadIdx.x;

    // own is uniform, so its map and its view are scalar loads; the corners are that instance's world corners, by the
    // formula every pair's are mapped with
    const float4 *own_row = maps + 3u * (uint32_t)own;
    const float4 own_map[3] = {own_row[0], own_row[1], own_row[2]};
    const SceneView &own_scene = leaf_view(records, views, own);
    const bool live = ta < own_scene.triangle_count;
    Query q;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            q.p[i][j] = 0.0f;
    if (live) {
        float c9[9];
        mapped_corners(own_map, own_scene.positions, ta, c9);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                q.p[i][j] = c9[3 * i + j];
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
    const int below = w.upper ? own : -1;   // SHRAY_PAIRS_UPPER: the instances up to own are not walked
    unsigned long long *const first_cells = w.first + (uint64_t)row * (uint64_t)w.n;
    unsigned long long *const count_cells = w.counts + (uint64_t)row * (uint64_t)w.n;   // (neither is dereferenced when null)
    unsigned int visited = 0, leaves = 0, tests = 0, walks = 0;

    if (__builtin_amdgcn_ballot_w64(walk)) {
        walk_top_level(
            nodes, top,
            // No axis separates the stored box from the query's vertex box, near zero by the guard's leave.  The root is not tested.
            [&](uint32_t node, const float4 &a, const float4 &b) { return walk && (node == 0u || stored_overlaps(a, b, q.lo, q.hi)); },
            // the lower child first (the walk's order affects its speed only)
            [&](uint32_t, uint32_t, unsigned long long) { return true; },
            [&](int inst, bool enters) {
                if (inst == own || inst <= below)   // (wave-uniform)
                    return;
                if (MODE == kAny && !COUNT) {
                    // skip (a): the cell is 1 already (every lane reads the one address)
                    if (__builtin_amdgcn_readfirstlane((int)cell_now(count_cells + inst)) != 0)
                        return;
                }
                if (MODE == kFirstOnly && !COUNT) {
                    // skip (b): a key of a smaller query triangle is in the cell, and this lane's keys all lie above it
                    enters = enters && (uint32_t)(cell_now(first_cells + inst) >> 32) >= ta;
                }
                const float4 *row_b = maps + 3u * (uint32_t)inst;
                const float4 m[3] = {row_b[0], row_b[1], row_b[2]};
                const SceneView &sc = leaf_view(records, views, inst);
                uint32_t members = 0, least = kNoTriangle;
                if (enters) {
                    walks++;
                    instance_walk<MODE == kAny>(sc, m, q, skip_shared, column, members, least, visited, leaves, tests);
                }
                // every lane of the wave is here again
                if (!__builtin_amdgcn_ballot_w64(members != 0))
                    return;
                if (MODE == kAny) {
                    if (threadIdx.x == 0)
                        atomicOr(count_cells + inst, 1ull);
                    return;
                }
                if (MODE == kCounts) {
                    const unsigned long long sum = wave_sum((unsigned long long)members);
                    if (threadIdx.x == 0)
                        atomicAdd(count_cells + inst, sum);
                }
                if (MODE == kFirstOnly || w.first) {
                    const unsigned long long key = wave_min(members ? ((unsigned long long)ta << 32) | least : kNone);
                    if (threadIdx.x == 0)
                        atomicMin(first_cells + inst, key);
                }
            });
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

constexpr uint32_t kFlags = SHRAY_PAIRS_ANY | SHRAY_PAIRS_SKIP_SHARED | SHRAY_PAIRS_UPPER;

// The refusals every form makes before it touches a device, in the header's order.
int check_query(const shray_instance_set *set, const shray_pairs_params *op, const void *first, const void *counts)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "pairs params are NULL");
    if (op->struct_size != sizeof(shray_pairs_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_pairs_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_pairs_params));
    if (op->flags & ~kFlags)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "pairs params out of range (flags 0x%x)", op->flags);
    if ((op->flags & SHRAY_PAIRS_ANY) && (first || !counts))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_PAIRS_ANY needs first NULL and counts");
    if (op->first_row < 0 || op->row_count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative first row %d or row count %d", op->first_row, op->row_count);
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    ShrayInstanceSetDevice d;
    if (const int rc = shrayi_instance_set_device_arrays(set, &d))
        return rc;
    if ((int64_t)op->first_row + (int64_t)op->row_count > (int64_t)d.count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "rows %d .. %lld are not all among the set's %d instances", op->first_row,
                    (long long)op->first_row + (long long)op->row_count, d.count);
    if (!first && !counts)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "nothing is asked for: first and counts are both NULL");
    if (!aligned(first, 8) || !aligned(counts, 8))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the keys and the counts must be 8-byte aligned");
    return SHRAY_OK;
}

// The table of the rows' workgroups, uint32 [rows + 1], and the rows' query triangles: from the members' triangle counts
// alone, read on the host.
int make_table(const shray_instance_set *set, const shray_pairs_params *op, std::vector<uint32_t> *table, uint64_t *triangles)
{
    table->assign((size_t)op->row_count + 1, 0u);
    uint64_t groups = 0;
    *triangles = 0;
    for (int32_t r = 0; r < op->row_count; r++) {
        shray_scene *scene = nullptr;
        ShrayQueryScene q;
        int rc = shrayi_instance_set_member_scene(set, op->first_row + r, &scene);
        if (rc || (rc = shrayi_scene_query_view(scene, &q)))
            return rc;
        (*table)[r] = (uint32_t)groups;
        groups += ((uint64_t)q.view.triangle_count + kBlock - 1) / kBlock;
        *triangles += q.view.triangle_count;
        if (groups > SHRAY_PAIRS_MAX_WORKGROUPS)
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "rows %d .. %d need more than the %u workgroups of one launch: take fewer rows per call",
                        op->first_row, op->first_row + op->row_count, SHRAY_PAIRS_MAX_WORKGROUPS);
    }
    (*table)[op->row_count] = (uint32_t)groups;
    return SHRAY_OK;
}

// Pinned host memory the table's copy reads from: kept by the library and taken again once the copy that read it has
// completed (the event is queried, never waited for), so the device form does not wait for the host.
struct Pinned {
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
    int device = -1;
};
std::mutex pinned_lock;
std::vector<Pinned> pinned;

int stage_table(const std::vector<uint32_t> &table, int device, uint32_t *d_table, hipStream_t stream)
{
    const size_t bytes = table.size() * sizeof(uint32_t);
    std::lock_guard<std::mutex> hold(pinned_lock);
    Pinned *use = nullptr;
    for (Pinned &p : pinned) {
        if (p.device != device || p.bytes < bytes)
            continue;
        if (hipEventQuery(p.copied) == hipSuccess) {
            use = &p;
            break;
        }
        (void)hipGetLastError();   // (hipErrorNotReady is an answer here, not an error for the launch after this)
    }
    if (!use) {
        Pinned p;
        p.device = device;
        p.bytes = bytes < 4096 ? 4096 : bytes;
        HIP_TRY(hipHostMalloc(&p.host, p.bytes, hipHostMallocDefault));
        const hipError_t e = hipEventCreateWithFlags(&p.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipHostFree(p.host);
            return fail(SHRAY_ERR_DEVICE, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        pinned.push_back(p);
        use = &pinned.back();
    }
    memcpy(use->host, table.data(), bytes);
    HIP_TRY(hipMemcpyAsync(d_table, use->host, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(use->copied, stream));
    return SHRAY_OK;
}

template <int MODE>
void launch(bool count, dim3 grid, size_t lds, hipStream_t stream, const PairsWork &w, const SetWalk &s)
{
    if (count)
        hipLaunchKernelGGL((instance_pairs_kernel<MODE, true>), grid, dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
    else
        hipLaunchKernelGGL((instance_pairs_kernel<MODE, false>), grid, dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
}

int pairs_device(shray_instance_set *set, const shray_pairs_params *op, uint64_t *d_first, int64_t *d_counts, hipStream_t stream,
                 DeviceCounters *d_counters, uint64_t *samples)
{
    int rc = check_query(set, op, d_first, d_counts);
    if (rc)
        return rc;
    if (samples)
        *samples = 0;
    if (op->row_count == 0)
        return SHRAY_OK;
    std::vector<uint32_t> table;
    uint64_t triangles = 0;
    if ((rc = make_table(set, op, &table, &triangles)))
        return rc;
    if (samples)
        *samples = triangles;
    return walk_set(set, true, 0, 0, nullptr, stream, [&](const SetWalk &s) {
        ShrayInstanceSetDevice d;
        if (const int code = shrayi_instance_set_device_arrays(set, &d))
            return code;
        const size_t cells = (size_t)op->row_count * (size_t)d.count;
        if (d_first)
            HIP_TRY(hipMemsetAsync(d_first, 0xff, cells * sizeof(uint64_t), stream));
        if (d_counts)
            HIP_TRY(hipMemsetAsync(d_counts, 0, cells * sizeof(int64_t), stream));
        const uint32_t groups = table.back();
        if (groups == 0)
            return (int)SHRAY_OK;
        uint32_t *d_table = nullptr;
        HIP_TRY(hipMallocAsync((void **)&d_table, table.size() * sizeof(uint32_t), stream));
        int code = stage_table(table, d.device, d_table, stream);
        if (!code) {
            const PairsWork w{(unsigned long long *)d_first,
                              (unsigned long long *)d_counts,
                              d_table,
                              op->first_row,
                              op->row_count,
                              d.count,
                              s.levels,
                              (op->flags & SHRAY_PAIRS_SKIP_SHARED) ? 1u : 0u,
                              (op->flags & SHRAY_PAIRS_UPPER) ? 1u : 0u,
                              d_counters};
            const size_t lds = s.lds(sizeof(uint32_t));
            if (op->flags & SHRAY_PAIRS_ANY)
                launch<kAny>(d_counters != nullptr, dim3(groups), lds, stream, w, s);
            else if (!d_counts)
                launch<kFirstOnly>(d_counters != nullptr, dim3(groups), lds, stream, w, s);
            else
                launch<kCounts>(d_counters != nullptr, dim3(groups), lds, stream, w, s);
            code = launched("instance-pair collision matrix");
        }
        const hipError_t e = hipFreeAsync(d_table, stream);
        if (e != hipSuccess && !code)
            code = fail(SHRAY_ERR_DEVICE, "hipFreeAsync failed: %s", hipGetErrorString(e));
        return code;
    });
}

// the blocking forms: the query on the null stream, the keys, counts (and tallies) back
int pairs_host(shray_instance_set *set, const shray_pairs_params *op, uint64_t *first, int64_t *counts, shray_counters *tallies)
{
    int rc = check_query(set, op, first, counts);
    if (rc)
        return rc;
    if (tallies)
        memset(tallies, 0, sizeof(*tallies));
    if (op->row_count == 0)
        return SHRAY_OK;
    if ((rc = enter_set(set)))   // the set's errors come before any allocation
        return rc;
    ShrayInstanceSetDevice d;
    if ((rc = shrayi_instance_set_device_arrays(set, &d)))
        return rc;
    const size_t cells = (size_t)op->row_count * (size_t)d.count;
    static const uint64_t no_items[2] = {};
    uint64_t samples = 0;
    rc = run_blocking({{no_items, 0}}, {{first, first ? cells * sizeof(uint64_t) : 0}, {counts, counts ? cells * sizeof(int64_t) : 0}}, tallies,
                      [&](DeviceBuffer *, DeviceBuffer *d_out, DeviceCounters *shards) {
                          return pairs_device(set, op, d_out[0].as<uint64_t>(), d_out[1].as<int64_t>(), nullptr, shards, &samples);
                      });
    if (!rc && tallies)
        tallies->samples = samples;
    return rc;
}

}   // namespace

static_assert(sizeof(shray_pairs_params) == 16, "shray_pairs_params is 16 bytes");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(unsigned long long) == sizeof(int64_t), "a cell is 8 bytes");

extern "C" {

int shray_instance_pairs_intersect_device(shray_instance_set *set, const shray_pairs_params *op, uint64_t *d_first, int64_t *d_counts,
                                          void *hip_stream)
{
    return pairs_device(set, op, d_first, d_counts, (hipStream_t)hip_stream, nullptr, nullptr);
}

int shray_instance_pairs_intersect(shray_instance_set *set, const shray_pairs_params *op, uint64_t *first, int64_t *counts)
{
    return pairs_host(set, op, first, counts, nullptr);
}

int shray_instance_pairs_intersect_counters(shray_instance_set *set, const shray_pairs_params *op, uint64_t *first, int64_t *counts,
                                            shray_counters *counters)
{
    if (!counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return pairs_host(set, op, first, counts, counters);
}

}   // extern "C"
