// instance_overlap.hip -- include/shader_ray_instance_overlap.h: every triangle of every instance of a set of placed scenes
// that touches each caller-supplied axis-aligned world box, counted, the K smallest (instance, triangle) pairs kept in order
// (DESIGN section 23).
//
// One lane per box in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level): a lane enters a node unless an axis separates the node's stored box from its query box, and near zero an
// axis may not separate (instance/image_box.h's kGuard; the stored box holds an instance's fp32 world corners only where the
// world coordinates are normal or 0).  At a leaf the instance is wave-uniform: its forward map's three rows and the member's SceneView come in
// by scalar loads, and the entering lanes run the box-overlap walk of overlap/overlap.hip over that member's packed tree with
// every box replaced by its image box under the map and every triangle's corners mapped before the 13-axis test.  A lane's K
// smallest carry from one instance into the next under the key (instance, triangle).
//
// The K smallest are kept as overlap.hip keeps them: in registers for K <= 8 (one 64-bit key a slot, every index a
// compile-time constant, no scratch), else the triangles in the box's own K output slots and the instances in the instance
// buffer beside them (instance/held_pairs.h's Held).  The image boxes, the corner mapping and the guard are
// instance/image_box.h's, the 13-axis test point/triangle_box_test.h's: this library compiles the code that
// libshray_instance_point.so and libshray_overlap.so compile.  It is built apart from libshray_hip.so and
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
#include "shader_ray_instance_overlap.h"
#include "top_level.h"
#include "trace_common.h"
#include "triangle_box_test.h"

using namespace shray;

namespace {

struct SetOverlapWork {
    const float4 *boxes;    // two per box: (lo, pad), (hi, pad), world space
    int32_t *out;           // k per box: triangles; not touched when k == 0
    int32_t *instances;     // k per box, or nullptr (never nullptr for the form that keeps its K smallest in memory, k > 0)
    int32_t *counts;        // one per box, or nullptr
    uint64_t count;
    uint64_t first;         // this launch's first box
    int32_t k;              // pairs per box
    int32_t stack_levels;   // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    DeviceCounters *counters;
};

// the pair (the instance whose map is m, triangle t of its scene): the corners mapped, then the 13-axis test
__device__ __forceinline__ bool mapped_overlaps(const float4 (&m)[3], const float *positions, uint32_t t, const float lo[3],
                                                const float hi[3], const float mid[3], const float h[3])
{
    return with_mapped_corners(m, positions, t, [&](const float *c9) { return triangle_overlaps(lo, hi, mid, h, c9); });
}

// One lane's walk of instance `inst`: overlap.hip's loop over the member's packed tree, on image boxes and mapped corners.
template <int SLOTS, bool ANY>
__device__ __forceinline__ void instance_walk(const SceneView &sc, const float4 (&m)[3], int inst, const float lo[3], const float hi[3],
                                              const float mid[3], const float h[3], uint32_t *column, Held<SLOTS> &held, int &n,
                                              unsigned int &nodes, unsigned int &leaves, unsigned int &tests)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    Record cur = load_record(copy, sc.packed_root);
    nodes++;
    int sp = 0;
    bool go = image_overlaps(m, cur.box, lo, hi);
    while (go) {
        if (cur.b & kLeafFlag) {
            leaves++;
            const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
            for (uint32_t t = first; t < first + in_leaf; t++) {
                tests++;
                if (!mapped_overlaps(m, sc.positions, t, lo, hi, mid, h))
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
            const bool in0 = image_overlaps(m, r0.box, lo, hi), in1 = image_overlaps(m, r1.box, lo, hi);
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

// One lane per box.  SLOTS: the register slots of the K smallest pairs (k <= SLOTS), kSlotsInMemory: they live in the box's
// output slots (any k, also 0).  PRUNE: a lane that holds K pairs skips an instance above all of them.  COUNT: the work
// counters.  ANY: a lane stops at its first touching pair (k is 0).  The pointers are __restrict__ so that a leaf's record,
// its map and its SceneView come in by scalar loads.
template <int SLOTS, bool PRUNE, bool COUNT, bool ANY>
__global__ void __launch_bounds__(kBlock) instance_overlap_kernel(SetOverlapWork w, const TopNode *__restrict__ nodes,
                                                                  const float4 *__restrict__ records, const float4 *__restrict__ maps,
                                                                  const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t overlap_stack[];
    uint32_t *column = overlap_stack + threadIdx.x;                        // level-major: a wave's accesses are consecutive
    uint32_t *top = overlap_stack + (size_t)kBlock * w.stack_levels;      // the wave's top-level stack
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = make_float4(-1.0f, -1.0f, -1.0f, 0.0f);
    if (live)
        b0 = w.boxes[2 * index], b1 = w.boxes[2 * index + 1];
    const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
    bool walk = live;
    float mid[3], h[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        walk = walk && __builtin_isfinite(lo[j]) && __builtin_isfinite(hi[j]) && !(lo[j] > hi[j]);
        mid[j] = 0.5f * lo[j] + 0.5f * hi[j];
        h[j] = 0.5f * hi[j] - 0.5f * lo[j];
    }
    const int k = w.k;

    Held<SLOTS> held;
    held.k = k;
    held.slots = w.out + index * (uint64_t)k;   // this box's own (dereferenced only when live and k > 0)
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
            // No axis separates the stored box from the query box, near zero by the guard's leave.  The root is not tested.
            [&](uint32_t node, const float4 &a, const float4 &b) {
                return walk && !(ANY && n > 0) && (node == 0u || stored_overlaps(a, b, lo, hi));
            },
            // the lower child first (the walk's order affects its speed only)
            [&](uint32_t, uint32_t, unsigned long long) { return true; },
            [&](int inst, bool enters) {
                const float4 *row = maps + 3u * (uint32_t)inst;
                const float4 m[3] = {row[0], row[1], row[2]};
                const SceneView &sc = leaf_view(records, views, inst);
                if (enters && !(PRUNE && held.full_below(inst))) {
                    walks++;
                    instance_walk<SLOTS, ANY>(sc, m, inst, lo, hi, mid, h, column, held, n, visited, leaves, tests);
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

constexpr Nouns kNouns = {"box", "boxes", "set", "out", "max_triangles", "instanced box-overlap query"};

// the checks every form makes before it touches a set or a device
int check_query(shray_instance_set *set, const shray_overlap_params *op, const void *boxes, int64_t count, const void *out,
                const void *instances, const void *counts)
{
    int rc = check_params(op);
    if (rc || (rc = check_any(op, counts)) || (rc = check_first_k(kNouns, set, boxes, count, op->max_triangles, out, counts)))
        return rc;
    if (!aligned(boxes, 16) || !aligned(out, 4) || !aligned(instances, 4) || !aligned(counts, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the boxes must be 16-byte aligned, the indices, the instances and the counts 4-byte aligned");
    return SHRAY_OK;
}

int overlap_device(shray_instance_set *set, const shray_overlap_params *op, const shray_box *d_boxes, int64_t count, int32_t *d_out,
                   int32_t *d_instances, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(set, op, d_boxes, count, d_out, d_instances, d_counts);
    if (rc)
        return rc;
    const int k = op->max_triangles;
    const bool any = (op->flags & SHRAY_OVERLAP_ANY) != 0;
    if (count == 0)
        return SHRAY_OK;
    return walk_set(set, true, k, count, d_instances, stream, [&](const SetWalk &s) {
        SetOverlapWork w{(const float4 *)d_boxes, k > 0 ? d_out : nullptr, k > 0 ? s.instances : nullptr, d_counts, (uint64_t)count, 0, k,
                         s.levels, d_counters};
        const size_t lds = s.lds(sizeof(uint32_t));
        return first_k_launches(kNouns, w, count, [&](dim3 grid) {
            if (any && d_counters)
                hipLaunchKernelGGL((instance_overlap_kernel<kSlotsInMemory, false, true, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else if (any)
                hipLaunchKernelGGL((instance_overlap_kernel<kSlotsInMemory, false, false, true>), grid, dim3(kBlock), lds, stream, w, s.nodes,
                                   s.records, s.maps, s.views);
            else
                with_slots(k, [&](auto slots) {
                    with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                        hipLaunchKernelGGL(
                            (instance_overlap_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value, false>), grid,
                            dim3(kBlock), lds, stream, w, s.nodes, s.records, s.maps, s.views);
                    });
                });
        });
    });
}

// the blocking forms: the boxes to the device, the query on the null stream, the indices, instances, counts (and tallies) back
int overlap_host(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes, int64_t count, int32_t *out,
                 int32_t *instances, int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(set, op, boxes, count, out, instances, counts))
        return rc;
    return first_k_blocking(
        {boxes, sizeof(shray_box), out, sizeof(int32_t), instances, counts}, count, op->max_triangles, tallies,
        [&] { return enter_set(set); },
        [&](void *d_boxes, void *d_out, int32_t *d_instances, int32_t *d_counts, DeviceCounters *shards) {
            return overlap_device(set, op, (const shray_box *)d_boxes, count, (int32_t *)d_out, d_instances, d_counts, nullptr, shards);
        });
}

}   // namespace

static_assert(sizeof(shray_overlap_params) == 16, "shray_overlap_params is 16 bytes");
static_assert(sizeof(shray_box) == 32, "shray_box is 32 bytes");

extern "C" {

int shray_overlap_triangles_instances_device(shray_instance_set *set, const shray_overlap_params *op, const shray_box *d_boxes,
                                             int64_t count, int32_t *d_out, int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return overlap_device(set, op, d_boxes, count, d_out, d_instances, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_overlap_triangles_instances(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes, int64_t count,
                                      int32_t *out, int32_t *instances, int32_t *counts)
{
    return overlap_host(set, op, boxes, count, out, instances, counts, nullptr);
}

int shray_overlap_triangles_instances_counters(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes,
                                               int64_t count, int32_t *out, int32_t *instances, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : overlap_host(set, op, boxes, count, out, instances, counts, counters);
}

}   // extern "C"
