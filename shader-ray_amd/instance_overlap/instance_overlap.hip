// instance_overlap.hip -- include/shader_ray_instance_overlap.h: every triangle of every instance of a set of placed scenes
// that touches each caller-supplied axis-aligned world box, counted, the K smallest (instance, triangle) pairs kept in order
// (DESIGN section 23).
//
// One lane per box in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level): a lane enters a node unless an axis separates the node's stored box from its query box, and near zero an
// axis may not separate (kGuard below; the stored box holds an instance's fp32 world corners only where the world coordinates
// are normal or 0).  At a leaf the instance is wave-uniform: its forward map's three rows and the member's SceneView come in
// by scalar loads, and the entering lanes run the box-overlap walk of overlap/overlap.hip over that member's packed tree with
// every box replaced by its image box under the map and every triangle's corners mapped before the 13-axis test.  A lane's K
// smallest carry from one instance into the next under the key (instance, triangle).
//
// The K smallest are kept as overlap.hip keeps them: in registers for K <= 8 (one 64-bit key a slot, every index a
// compile-time constant, no scratch), else the triangles in the box's own K output slots and the instances in the instance
// buffer beside them.  image_box and the corner mapping restate instance_point/instance_point.hip's, min3 .. triangle_overlaps
// restate overlap.hip's: moving them to a header would put those libraries' units on another include path.
// This library is built apart from libshray_hip.so, libshray_instance.so, libshray_overlap.so and libshray_instance_point.so,
// so their code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "client_internal.h"
#include "enter_set.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "shader_ray_instance_overlap.h"
#include "top_level.h"
#include "trace_common.h"

using namespace shray;

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;   // after every (instance, triangle)

// Below this magnitude a stored top-level float and the query float beside it may not separate an axis.  place_box's margin,
// 128 u s (|Y| + |b|), covers the three half subnormal steps by which an fp32 corner can leave its exact image as soon as the
// box's largest coordinate reaches 2^-109 (DESIGN sections 20 and 23), so a corner outside its stored box, the stored end it
// passed and any query end between the two are all below 2^-109.
constexpr float kGuard = 0x1p-109f;

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

// include/shader_ray_overlap.h's min and max: comparisons, so that a NaN is passed on or dropped as the header's are
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

// include/shader_ray_overlap.h's per-triangle test: the box (lo, hi), its centre m and half extent h, nine world floats
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

// the image of a node's box under the map's rows: per world axis the corner formula on the ends that make it smallest and
// largest, chosen by the signs of the row's entries alone (a zero entry is not read: either end)
__device__ __forceinline__ Box image_box(const float4 (&m)[3], const Box &b)
{
    Box o;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float row[3] = {m[r].x, m[r].y, m[r].z};
        float lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = row[c] < 0.0f ? b.hi[c] : b.lo[c];
            hi[c] = row[c] < 0.0f ? b.lo[c] : b.hi[c];
        }
        o.lo[r] = object_row(m[r], mk(lo[0], lo[1], lo[2]), true);
        o.hi[r] = object_row(m[r], mk(hi[0], hi[1], hi[2]), true);
    }
    return o;
}

// a member node's cull: its image box against the query box, six comparisons; a NaN end compares false and culls less
__device__ __forceinline__ bool image_overlaps(const float4 (&m)[3], const Box &node, const float lo[3], const float hi[3])
{
    const Box o = image_box(m, node);
    return !(o.hi[0] < lo[0] || o.lo[0] > hi[0] || o.hi[1] < lo[1] || o.lo[1] > hi[1] || o.hi[2] < lo[2] || o.lo[2] > hi[2]);
}

// one comparison of a top-level node's cull: the stored end lies beyond the query end, and the two are not both near zero
__device__ __forceinline__ bool guarded(bool beyond, float stored, float query)
{
    return beyond && !(fabsf(stored) < kGuard && fabsf(query) < kGuard);
}

// a top-level node's cull: its stored box (a, b) against the query box
__device__ __forceinline__ bool stored_overlaps(const float4 &a, const float4 &b, const float lo[3], const float hi[3])
{
    return !(guarded(b.x < lo[0], b.x, lo[0]) || guarded(a.x > hi[0], a.x, hi[0]) || guarded(b.y < lo[1], b.y, lo[1]) ||
             guarded(a.y > hi[1], a.y, hi[1]) || guarded(b.z < lo[2], b.z, lo[2]) || guarded(a.z > hi[2], a.z, hi[2]));
}

// the pair (the instance whose map is m, triangle t of its scene): the corners mapped, then the 13-axis test
__device__ __forceinline__ bool mapped_overlaps(const float4 (&m)[3], const float *positions, uint32_t t, const float lo[3],
                                                const float hi[3], const float mid[3], const float h[3])
{
    const float *v = positions + 9ull * t;
    float c9[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V3 corner = mk(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
#pragma unroll
        for (int r = 0; r < 3; r++)
            c9[3 * k + r] = object_row(m[r], corner, true);
    }
    return triangle_overlaps(lo, hi, mid, h, c9);
}

__device__ __forceinline__ unsigned long long key_of(int inst, uint32_t tri) { return ((unsigned long long)(uint32_t)inst << 32) | tri; }

// A lane's K smallest.  SLOTS > 0: the keys in registers, ascending; kSlotsInMemory: the triangles in the box's own output
// slots and their instances beside them (any k, also 0).
template <int SLOTS>
struct Held {
    static constexpr int R = SLOTS > 0 ? SLOTS : 1;
    unsigned long long key[R];   // (plain scalars: every index is a constant once unrolled)
    int32_t *slots;              // in memory: this box's own triangles and instances (dereferenced only when live and k > 0)
    int32_t *slot_inst;
    int k;

    // the pair sinks to where it sorts, the largest falls off
    __device__ __forceinline__ void insert(int inst, uint32_t t)
    {
        if (SLOTS != kSlotsInMemory) {
            unsigned long long carry = key_of(inst, t);
#pragma unroll
            for (int i = 0; i < R; i++) {
                const unsigned long long low = carry < key[i] ? carry : key[i];
                carry = carry < key[i] ? key[i] : carry;
                key[i] = low;
            }
        } else if (k > 0 && before(inst, t, slot_inst[k - 1], slots[k - 1])) {
            int i = k - 1;
            while (i > 0) {
                const int32_t st = slots[i - 1], si = slot_inst[i - 1];
                if (!before(inst, t, si, st))
                    break;
                slots[i] = st, slot_inst[i] = si;
                i--;
            }
            slots[i] = (int32_t)t, slot_inst[i] = inst;
        }
    }

    // the key of the header against a slot in memory; an empty slot (triangle < 0) is after every pair
    static __device__ __forceinline__ bool before(int inst, uint32_t t, int32_t slot_inst, int32_t slot_tri)
    {
        return slot_tri < 0 || inst < slot_inst || (inst == slot_inst && t < (uint32_t)slot_tri);
    }

    // whether K pairs are held and every one of them is of an instance below `inst`: no pair of `inst` can be among the K
    // smallest, because the key leads with the instance
    __device__ __forceinline__ bool full_below(int inst) const
    {
        if (SLOTS != kSlotsInMemory) {
            unsigned long long last = kEmptyKey;
#pragma unroll
            for (int i = 0; i < R; i++)
                last = i == k - 1 ? key[i] : last;
            return last != kEmptyKey && (uint32_t)inst > (uint32_t)(last >> 32);
        }
        return k > 0 && slots[k - 1] >= 0 && inst > slot_inst[k - 1];
    }
};

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

// include/shader_ray_overlap.h's params check, with the misuse of SHRAY_OVERLAP_ANY (overlap/overlap.hip makes the same two)
int check_params(const shray_overlap_params *op, const void *counts)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params are NULL");
    if (op->struct_size != sizeof(shray_overlap_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_overlap_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_overlap_params));
    if (op->max_triangles < 0 || op->max_triangles > SHRAY_OVERLAP_MAX || (op->flags & ~(uint32_t)SHRAY_OVERLAP_ANY) || op->reserved != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params out of range (max_triangles %d of 0 .. %d, flags 0x%x, reserved %d)",
                    op->max_triangles, (int)SHRAY_OVERLAP_MAX, op->flags, op->reserved);
    if ((op->flags & SHRAY_OVERLAP_ANY) && (op->max_triangles != 0 || !counts))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_OVERLAP_ANY needs max_triangles 0 (it is %d) and counts", op->max_triangles);
    return SHRAY_OK;
}

// the checks every form makes before it touches a set or a device
int check_query(shray_instance_set *set, const shray_overlap_params *op, const void *boxes, int64_t count, const void *out,
                const void *instances, const void *counts)
{
    int rc = check_params(op, counts);
    if (rc || (rc = check_first_k(kNouns, set, boxes, count, op->max_triangles, out, counts)))
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
    ShrayInstanceSetDevice d;
    int height = 0;
    if ((rc = enter_set(set, &d, &height)))
        return rc;
    const float *d_maps = nullptr;
    if ((rc = shrayi_instance_set_forward_maps(set, stream, &d_maps)))
        return rc;
    // the form that keeps its K smallest in the box's output slots keeps the instance half of the keys beside them: without an
    // instance buffer of the caller's, in scratch that is taken and given back in stream order
    int32_t *scratch = nullptr;
    if (kept_in_memory(k) && !d_instances) {
        HIP_TRY(hipMallocAsync((void **)&scratch, (size_t)count * (size_t)k * sizeof(int32_t), stream));
        d_instances = scratch;
    }
    const int levels = (int)stack_levels(height);
    SetOverlapWork w{(const float4 *)d_boxes, k > 0 ? d_out : nullptr, k > 0 ? d_instances : nullptr, d_counts, (uint64_t)count, 0, k, levels,
                     d_counters};
    const size_t lds = (size_t)kBlock * (size_t)levels * sizeof(uint32_t) + kTopStack * sizeof(uint32_t);
    const TopNode *nodes = static_cast<const TopNode *>(d.nodes);
    const float4 *records = static_cast<const float4 *>(d.records);
    const float4 *maps = reinterpret_cast<const float4 *>(d_maps);
    const SceneView *views = static_cast<const SceneView *>(d.views);
    rc = first_k_launches(kNouns, w, count, [&](dim3 grid) {
        if (any && d_counters)
            hipLaunchKernelGGL((instance_overlap_kernel<kSlotsInMemory, false, true, true>), grid, dim3(kBlock), lds, stream, w, nodes, records,
                               maps, views);
        else if (any)
            hipLaunchKernelGGL((instance_overlap_kernel<kSlotsInMemory, false, false, true>), grid, dim3(kBlock), lds, stream, w, nodes, records,
                               maps, views);
        else
            with_slots(k, [&](auto slots) {
                with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                    hipLaunchKernelGGL((instance_overlap_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value, false>),
                                       grid, dim3(kBlock), lds, stream, w, nodes, records, maps, views);
                });
            });
    });
    if (scratch) {
        const hipError_t e = hipFreeAsync(scratch, stream);
        if (e != hipSuccess && !rc)
            rc = fail(SHRAY_ERR_DEVICE, "hipFreeAsync failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// the blocking forms: the boxes to the device, the query on the null stream, the indices, instances, counts (and tallies) back
int overlap_host(shray_instance_set *set, const shray_overlap_params *op, const shray_box *boxes, int64_t count, int32_t *out,
                 int32_t *instances, int32_t *counts, shray_counters *tallies)
{
    if (const int rc = check_query(set, op, boxes, count, out, instances, counts))
        return rc;
    return first_k_blocking(
        {boxes, sizeof(shray_box), out, sizeof(int32_t), instances, counts}, count, op->max_triangles, tallies,
        [&] {
            ShrayInstanceSetDevice d;
            int height = 0;
            return enter_set(set, &d, &height);
        },
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
