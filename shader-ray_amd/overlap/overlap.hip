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
// index is a compile-time constant, so there is no scratch), else in the box's own K output slots.
// This library is built apart from libshray_hip.so, so the renderer's and the other clients' code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "shader_ray_overlap.h"

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

// the header's min and max: comparisons, so that a NaN is passed on or dropped as the header's are
__device__ __forceinline__ float min2(float x, float y) { return x < y ? x : y; }
__device__ __forceinline__ float max2(float x, float y) { return x > y ? x : y; }
__device__ __forceinline__ float min3(float x, float y, float z) { return min2(min2(x, y), z); }
__device__ __forceinline__ float max3(float x, float y, float z) { return max2(max2(x, y), z); }

// one edge axis of stage 2: the corners' projections p0, p1, p2 against the box's radius r
__device__ __forceinline__ bool separated(float p0, float p1, float p2, float r)
{
    return min3(p0, p1, p2) > r || max3(p0, p1, p2) < -r;
}

// the three axes (edge x box axis) of one edge e over the corners v0, v1, v2
__device__ __forceinline__ bool edge_separates(const float e[3], const float v0[3], const float v1[3], const float v2[3], const float h[3])
{
    const float ax = fabsf(e[0]), ay = fabsf(e[1]), az = fabsf(e[2]);
    if (separated(e[1] * v0[2] - e[2] * v0[1], e[1] * v1[2] - e[2] * v1[1], e[1] * v2[2] - e[2] * v2[1], h[1] * az + h[2] * ay))
        return true;
    if (separated(e[2] * v0[0] - e[0] * v0[2], e[2] * v1[0] - e[0] * v1[2], e[2] * v2[0] - e[0] * v2[2], h[0] * az + h[2] * ax))
        return true;
    return separated(e[0] * v0[1] - e[1] * v0[0], e[0] * v1[1] - e[1] * v1[0], e[0] * v2[1] - e[1] * v2[0], h[0] * ay + h[1] * ax);
}

// the header's per-triangle test: the box (lo, hi), its centre m and half extent h, the triangle's nine floats
__device__ __forceinline__ bool triangle_overlaps(const float lo[3], const float hi[3], const float m[3], const float h[3], const float *tri)
{
    float a[3], b[3], c[3];
#pragma unroll
    for (int j = 0; j < 3; j++)
        a[j] = tri[j], b[j] = tri[3 + j], c[j] = tri[6 + j];
    // stage 0: the box's axes, on the untranslated coordinates
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (min3(a[j], b[j], c[j]) > hi[j] || max3(a[j], b[j], c[j]) < lo[j])
            return false;
    float v0[3], v1[3], v2[3], e0[3], e1[3], e2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        v0[j] = a[j] - m[j], v1[j] = b[j] - m[j], v2[j] = c[j] - m[j];
        e0[j] = v1[j] - v0[j], e1[j] = v2[j] - v1[j], e2[j] = v0[j] - v2[j];
    }
    // stage 1: the triangle's plane
    const float nx = e0[1] * e1[2] - e0[2] * e1[1], ny = e0[2] * e1[0] - e0[0] * e1[2], nz = e0[0] * e1[1] - e0[1] * e1[0];
    const float d = (nx * v0[0] + ny * v0[1]) + nz * v0[2];
    const float r = (h[0] * fabsf(nx) + h[1] * fabsf(ny)) + h[2] * fabsf(nz);
    if (d > r || d < -r)
        return false;
    // stage 2: edge x box axis
    return !(edge_separates(e0, v0, v1, v2, h) || edge_separates(e1, v0, v1, v2, h) || edge_separates(e2, v0, v1, v2, h));
}

// the walk's cull: the node's box against the query box, six comparisons of stored floats
__device__ __forceinline__ bool boxes_overlap(const Box &node, const float lo[3], const float hi[3])
{
    return !(node.hi[0] < lo[0] || node.lo[0] > hi[0] || node.hi[1] < lo[1] || node.lo[1] > hi[1] || node.hi[2] < lo[2] ||
             node.lo[2] > hi[2]);
}

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

int check_params(const shray_overlap_params *op)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params are NULL");
    if (op->struct_size != sizeof(shray_overlap_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_overlap_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_overlap_params));
    if (op->max_triangles < 0 || op->max_triangles > SHRAY_OVERLAP_MAX || (op->flags & ~(uint32_t)SHRAY_OVERLAP_ANY) || op->reserved != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params out of range (max_triangles %d of 0 .. %d, flags 0x%x, reserved %d)",
                    op->max_triangles, (int)SHRAY_OVERLAP_MAX, op->flags, op->reserved);
    return SHRAY_OK;
}

// the checks every form makes before it touches a scene or a device
int check_query(shray_scene *scene, const shray_overlap_params *op, const void *boxes, int64_t count, const void *out, const void *counts)
{
    const int rc = check_params(op);
    if (rc)
        return rc;
    return check_first_k(kNouns, scene, boxes, count, op->max_triangles, out, counts, [&] {
        if ((op->flags & SHRAY_OVERLAP_ANY) && (op->max_triangles != 0 || !counts))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_OVERLAP_ANY needs max_triangles 0 (it is %d) and counts", op->max_triangles);
        return (int)SHRAY_OK;
    });
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
