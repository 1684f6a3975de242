// overlap.hip -- include/shader_ray_overlap.h: every triangle of a resident scene that touches each caller-supplied
// axis-aligned box, counted, the K smallest indices kept in order.
//
// One lane per box in one-wave workgroups.  The walk reads the 32-byte records of octant copy 7 of the packed tree
// (point/packed_walk.h) and the corners from the scene's positions; its stack is a level-major LDS column of node names, one
// entry per edge of the tree's height.  A node is entered iff its box overlaps the query box on all three axes: six
// comparisons of stored floats, exact because stage 0 of the header's test is the same comparison on the triangle's own
// vertex box and a node's box is the min/max of the vertices below it.  Every triangle of a visited leaf takes the header's
// 13-axis test, in index order.  The set does not depend on the visit order (the header).
//
// The K smallest indices are kept by sorted insertion: in registers for K <= 8 (instances for 1, 2, 4 and 8 slots; every
// index is a compile-time constant, so there is no scratch), else in the box's own K output slots.  The per-triangle test
// and the cull are point/triangle_box_test.h's, which the instanced form compiles too.
// This library is built apart from libshray_hip.so, so the renderer's and the other clients' code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "params_check.h"
#include "shader_ray_overlap.h"
#include "triangle_box_test.h"

using namespace shray;

namespace {

constexpr uint32_t kEmpty = 0xffffffffu;   // SHRAY_HIT_MISS as an unsigned index: after every triangle

struct OverlapWork {
    const float4 *boxes;   // two per box: (lo, pad), (hi, pad)
    int32_t *out;          // k per box; not touched when k == 0
    int32_t *counts;       // one per box, or nullptr
    uint64_t count;
    uint64_t first;        // this launch's first box
    int32_t k;             // indices per box
    DeviceCounters *counters;
};

// One lane per box.  SLOTS: the register slots of the K smallest indices (k <= SLOTS), kSlotsInMemory: they live in the
// box's output slots (any k, also 0).  ANY: stop at the first overlapping triangle (k is 0).  COUNT: the work counters.
template <int SLOTS, bool ANY, bool COUNT>
__global__ void __launch_bounds__(kBlock) overlap_kernel(SceneView sc, OverlapWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t overlap_stack[];
    uint32_t *column = overlap_stack + threadIdx.x;   // level-major: a wave's accesses are consecutive
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = make_float4(-1.0f, -1.0f, -1.0f, 0.0f);
    if (live)
        b0 = w.boxes[2 * index], b1 = w.boxes[2 * index + 1];
    const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
    bool walk = live;
    float m[3], h[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        walk = walk && __builtin_isfinite(lo[j]) && __builtin_isfinite(hi[j]) && !(lo[j] > hi[j]);
        m[j] = 0.5f * lo[j] + 0.5f * hi[j];
        h[j] = 0.5f * hi[j] - 0.5f * lo[j];
    }
    const int k = w.k;
    int32_t *slots = w.out + index * (uint64_t)k;   // this box's own (dereferenced only when live and k > 0)

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
        bool go = boxes_overlap(cur.box, lo, hi);
        while (go) {
            if (cur.b & kLeafFlag) {
                leaves++;
                const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
                for (uint32_t t = first; t < first + in_leaf; t++) {
                    tests++;
                    if (!triangle_overlaps(lo, hi, m, h, sc.positions + 9ull * t))
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
                const bool in0 = boxes_overlap(r0.box, lo, hi), in1 = boxes_overlap(r1.box, lo, hi);
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

constexpr Nouns kNouns = {"box", "boxes", "scene", "out", "max_triangles", "box-overlap query"};

// the checks every form makes before it touches a scene or a device
int check_query(shray_scene *scene, const shray_overlap_params *op, const void *boxes, int64_t count, const void *out, const void *counts)
{
    const int rc = check_params(op);
    if (rc)
        return rc;
    return check_first_k(kNouns, scene, boxes, count, op->max_triangles, out, counts, [&] { return check_any(op, counts); });
}

// (this walk has no form that prunes: the choice is the work counters alone)
template <int SLOTS>
void launch_form(dim3 grid, size_t lds, hipStream_t stream, const SceneView &view, const OverlapWork &w)
{
    if (w.counters)
        hipLaunchKernelGGL((overlap_kernel<SLOTS, false, true>), grid, dim3(kBlock), lds, stream, view, w);
    else
        hipLaunchKernelGGL((overlap_kernel<SLOTS, false, false>), grid, dim3(kBlock), lds, stream, view, w);
}

int overlap_device(shray_scene *scene, const shray_overlap_params *op, const shray_box *d_boxes, int64_t count, int32_t *d_out,
                   int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(scene, op, d_boxes, count, d_out, d_counts);
    if (rc)
        return rc;
    const int k = op->max_triangles;
    const bool any = (op->flags & SHRAY_OVERLAP_ANY) != 0;
    if (!aligned(d_boxes, 16) || (k > 0 && !aligned(d_out, 4)) || (d_counts && !aligned(d_counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the boxes must be 16-byte aligned, the indices and the counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))
        return rc;
    OverlapWork w{(const float4 *)d_boxes, k > 0 ? d_out : nullptr, d_counts, (uint64_t)count, 0, k, d_counters};
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint32_t);
    return first_k_launches(kNouns, w, count, [&](dim3 grid) {
        if (any && d_counters)
            hipLaunchKernelGGL((overlap_kernel<kSlotsInMemory, true, true>), grid, dim3(kBlock), lds, stream, q.view, w);
        else if (any)
            hipLaunchKernelGGL((overlap_kernel<kSlotsInMemory, true, false>), grid, dim3(kBlock), lds, stream, q.view, w);
        else
            with_slots(k, [&](auto slots) { launch_form<decltype(slots)::value>(grid, lds, stream, q.view, w); });
    });
}

// the blocking forms: the boxes to the device, the query on the null stream, the indices, counts (and tallies) back
int overlap_host(shray_scene *scene, const shray_overlap_params *op, const shray_box *boxes, int64_t count, int32_t *out, int32_t *counts,
                 shray_counters *tallies)
{
    if (const int rc = check_query(scene, op, boxes, count, out, counts))
        return rc;
    if (!aligned(boxes, 16) || (out && !aligned(out, 4)) || (counts && !aligned(counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the boxes must be 16-byte aligned, the indices and the counts 4-byte aligned");
    return first_k_blocking(
        {boxes, sizeof(shray_box), out, sizeof(int32_t), nullptr, counts}, count, op->max_triangles, tallies,
        [&] {
            ShrayQueryScene q;
            int height = 0;
            return enter_walkable_scene(scene, &q, &height);
        },
        [&](void *d_boxes, void *d_out, int32_t *, int32_t *d_counts, DeviceCounters *shards) {
            return overlap_device(scene, op, (const shray_box *)d_boxes, count, (int32_t *)d_out, d_counts, nullptr, shards);
        });
}

}   // namespace

static_assert(sizeof(shray_overlap_params) == 16, "shray_overlap_params is 16 bytes");
static_assert(sizeof(shray_box) == 32, "shray_box is 32 bytes");

extern "C" {

void shray_overlap_params_init(shray_overlap_params *op)
{
    if (!op)
        return;
    op->struct_size = sizeof(shray_overlap_params);
    op->max_triangles = 8;
    op->flags = 0;
    op->reserved = 0;
}

int shray_overlap_triangles_device(shray_scene *scene, const shray_overlap_params *op, const shray_box *d_boxes, int64_t count,
                                   int32_t *d_out, int32_t *d_counts, void *hip_stream)
{
    return overlap_device(scene, op, d_boxes, count, d_out, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_overlap_triangles(shray_scene *scene, const shray_overlap_params *op, const shray_box *boxes, int64_t count, int32_t *out,
                            int32_t *counts)
{
    return overlap_host(scene, op, boxes, count, out, counts, nullptr);
}

int shray_overlap_triangles_counters(shray_scene *scene, const shray_overlap_params *op, const shray_box *boxes, int64_t count,
                                     int32_t *out, int32_t *counts, shray_counters *counters)
{
    const int rc = check_counters(counters);
    return rc ? rc : overlap_host(scene, op, boxes, count, out, counts, counters);
}

}   // extern "C"
