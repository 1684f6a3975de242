// multihit.hip -- include/shader_ray_multihit.h: every crossing of a caller-supplied ray with a resident scene, counted, the
// first K kept in order.
//
// One lane per ray in one-wave workgroups.  The walk reads the 32-byte records of octant copy 7 of the packed tree
// (packed_layout.h: entry planes = boxmin, exit planes = boxmax; the slab test selects per axis by d >= 0, as the shader's
// range_intersect_box does) and the corners from the scene's positions.  Its stack lies in LDS, level-major, one entry per
// edge of the tree's height, as point/point_walk.h's (point/packed_walk.h has what the two walks share).  The crossing set does not depend on the visit order (the header), so
// the walk visits the child with the smaller r0 first, and the form that is not asked for counts skips a node whose r0 is
// above the K-th smallest t held: nothing in it can enter the first K.
//
// The K best are kept by sorted insertion: in registers for K <= 8 (instances for 1, 2, 4 and 8 slots; every index is a
// compile-time constant, so there is no scratch), in the ray's own K output slots for larger K.
// This library is built apart from libshray_hip.so, so the renderer's code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "client_internal.h"
#include "exact_div.h"
#include "packed_walk.h"
#include "shader_ray_multihit.h"
#include "trace_common.h"

using namespace shray;

namespace {

constexpr uint64_t kRaysPerLaunch = 1ull << 24;   // the grid's threads stay far below 2^32
constexpr float kDetEps = 0.0000001f;             // fs:311
constexpr int kSlotsInMemory = 0;                 // SLOTS of the instance that keeps its K best in the ray's output slots

struct MultiWork {
    const float4 *rays;   // 2 float4 per ray
    float4 *hits;         // k per ray: (t, u, v, triangle bits); not touched when k == 0
    int32_t *counts;      // one per ray, or nullptr
    uint64_t count;
    uint64_t first;       // this launch's first ray
    int32_t k;            // records per ray
    int32_t max_leaf_tests;
    DeviceCounters *counters;
};

// the key of the header: t as a float comparison, then the triangle index
__device__ __forceinline__ bool before(float t, int tri, float slot_t, int slot_tri)
{
    return t < slot_t || (t == slot_t && tri < slot_tri);
}
__device__ __forceinline__ bool before(float t, int tri, float4 slot) { return before(t, tri, slot.x, __float_as_int(slot.w)); }

// a ray's divisors: its direction, and where exact_div.h's conditions hold the correctly rounded reciprocals
struct Slab {
    float o[3], d[3], y[3], yl[3];
    bool exact;   // every quotient of this ray may take div_by_constant4
};

__device__ __forceinline__ Slab make_slab(const SceneView &sc, V3 P, V3 D)
{
    Slab s;
    s.o[0] = P.x, s.o[1] = P.y, s.o[2] = P.z;
    s.d[0] = D.x, s.d[1] = D.y, s.d[2] = D.z;
    s.exact = sc.exact_div_ok != 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s.exact = s.exact && divisor_in_range(s.d[a]) && coordinate_in_range(s.o[a]);
        s.y[a] = reciprocal_in_range(s.d[a]);   // (not looked at when the ray is not exact)
        s.yl[a] = reciprocal_residual(s.d[a], s.y[a]);
    }
    return s;
}

// range_intersect_box over [0, 1e8] (fs:200-217): true divisions, or their exact_div.h equals
__device__ __forceinline__ void slab_range(const Slab &s, const Box &b, float &r0, float &r1)
{
    float ta[3], tb[3];
    if (s.exact) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            ta[a] = div_by_constant4(b.lo[a] - s.o[a], s.d[a], s.y[a], s.yl[a]);
            tb[a] = div_by_constant4(b.hi[a] - s.o[a], s.d[a], s.y[a], s.yl[a]);
        }
    } else {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            ta[a] = (b.lo[a] - s.o[a]) / s.d[a];
            tb[a] = (b.hi[a] - s.o[a]) / s.d[a];
        }
    }
    r0 = 0.0f, r1 = kRangeMax;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool forward = s.d[a] >= 0.0f;
        r0 = sel_max(r0, forward ? ta[a] : tb[a]);
        r1 = sel_min(r1, forward ? tb[a] : ta[a]);
    }
}

// One lane per ray.  SLOTS: the register slots of the K best (k <= SLOTS), kSlotsInMemory: they live in the ray's output
// slots (any k, also 0).  PRUNE: skip nodes that cannot reach the first k (no count is written).  COUNT: the work counters.
template <int SLOTS, bool PRUNE, bool COUNT>
__global__ void __launch_bounds__(kBlock) all_hits_kernel(SceneView sc, MultiWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    uint32_t *column = lds_stack + threadIdx.x;   // node names, level-major
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (live) {
        ra = w.rays[2 * index];
        rb = w.rays[2 * index + 1];
    }
    const V3 P = mk(ra.x, ra.y, ra.z), D = mk(rb.x, rb.y, rb.z);
    const float tmax = ra.w;
    const bool traced = live && tmax > 0.0f;   // (false for NaN)
    const int k = w.k;
    const float4 empty = make_float4(tmax, 0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS));
    float4 *slots = w.hits + index * (uint64_t)k;   // this ray's own (dereferenced only when live and k > 0)

    constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float held_t[R], held_u[R], held_v[R];   // (plain scalars: every index below is a constant once unrolled)
    int held_tri[R];
#pragma unroll
    for (int i = 0; i < R; i++)
        held_t[i] = tmax, held_u[i] = 0.0f, held_v[i] = 0.0f, held_tri[i] = SHRAY_HIT_MISS;
    if (SLOTS == kSlotsInMemory && live)
        for (int i = 0; i < k; i++)
            slots[i] = empty;
    // the k-th smallest t held; tmax while fewer than k are held (an accepted t is below tmax, and so is an entered r0)
    float tk = tmax;
    int n = 0;
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};

    if (traced) {
        const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
        const Slab slab = make_slab(sc, P, D);
        rc.traversals = 1;
        Record cur = load_record(copy, sc.packed_root);
        float r0, r1;
        slab_range(slab, cur.box, r0, r1);
        rc.node_visits = 1;
        rc.leaf_visits = (cur.b & kLeafFlag) ? 1 : 0;
        int sp = 0;
        bool go = !(r0 >= r1) && r0 < tmax;
        while (go) {
            if (cur.b & kLeafFlag) {
                const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
                const uint32_t tests = in_leaf < (uint32_t)w.max_leaf_tests ? in_leaf : (uint32_t)w.max_leaf_tests;
                for (uint32_t j = 0; j < tests; j++) {
                    rc.triangle_tests++;
                    const int tri = (int)(first + j);
                    const float *v = sc.positions + 9ull * (uint32_t)tri;
                    const V3 v0 = mk(v[0], v[1], v[2]), v1 = mk(v[3], v[4], v[5]), v2 = mk(v[6], v[7], v[8]);
                    const V3 e0 = v1 - v0, e1 = v0 - v2;
                    const V3 M = cross3(e1, D);
                    const float det = dot3(e0, M);
                    if (det > -kDetEps && det < kDetEps)
                        continue;
                    const float inv_det = 1.0f / det;
                    const V3 T = P - v0;
                    const V3 Q = cross3(T, e0);
                    const float dist = -dot3(e1, Q) * inv_det;
                    if (dist > tmax || dist < r0 || dist > r1)
                        continue;
                    const float u = dot3(T, M) * inv_det;
                    if (u < 0.0f || u > 1.0f)
                        continue;
                    const float bw = dot3(D, Q) * inv_det;
                    if (bw < 0.0f || u + bw > 1.0f)
                        continue;
                    if (!(dist < tmax))   // the report rule; NaN ends here too
                        continue;
                    n++;
                    if (SLOTS != kSlotsInMemory) {
                        // the record moves in where it sorts, the rest move down, the last falls off
#pragma unroll
                        for (int i = R - 1; i >= 0; i--) {
                            constexpr int kNone = 0;
                            const int up = i > 0 ? i - 1 : kNone;
                            const bool here = before(dist, tri, held_t[i], held_tri[i]);
                            const bool above = i > 0 && before(dist, tri, held_t[up], held_tri[up]);
                            held_t[i] = above ? held_t[up] : (here ? dist : held_t[i]);
                            held_u[i] = above ? held_u[up] : (here ? u : held_u[i]);
                            held_v[i] = above ? held_v[up] : (here ? bw : held_v[i]);
                            held_tri[i] = above ? held_tri[up] : (here ? tri : held_tri[i]);
                        }
#pragma unroll
                        for (int i = 0; i < R; i++)
                            tk = i == k - 1 ? held_t[i] : tk;
                    } else if (k > 0 && before(dist, tri, slots[k - 1])) {
                        int i = k - 1;
                        while (i > 0) {
                            const float4 s = slots[i - 1];
                            if (!before(dist, tri, s))
                                break;
                            slots[i] = s;
                            i--;
                        }
                        slots[i] = make_float4(dist, u, bw, __int_as_float(tri));
                        tk = slots[k - 1].x;
                    }
                }
            } else {
                const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                const Record c0 = load_record(copy, n0), c1 = load_record(copy, n1);
                float a0, b0, a1, b1;
                slab_range(slab, c0.box, a0, b0);
                slab_range(slab, c1.box, a1, b1);
                rc.node_visits += 2;
                rc.leaf_visits += ((c0.b & kLeafFlag) ? 1 : 0) + ((c1.b & kLeafFlag) ? 1 : 0);
                // entered (the header); skipped when nothing in it can reach the first k: an accepted t is never below
                // its leaf's r0, a descendant's r0 never below this one (a NaN r0 compares false: visited)
                const bool e0 = !(a0 >= b0) && a0 < tmax && !(PRUNE && a0 > tk);
                const bool e1 = !(a1 >= b1) && a1 < tmax && !(PRUNE && a1 > tk);
                const bool second = a1 < a0;   // the child with the smaller r0 first
                const bool go_near = second ? e1 : e0, go_far = second ? e0 : e1;
                if (go_near || go_far) {
                    if (go_near && go_far) {
                        column[(size_t)sp * kBlock] = second ? n0 : n1;
                        sp++;
                    }
                    const bool take1 = go_near ? second : !second;
                    cur = take1 ? c1 : c0;
                    r0 = take1 ? a1 : a0;
                    r1 = take1 ? b1 : b0;
                    continue;
                }
            }
            // the next pending node; the stack holds at most one entry per level of the current path
            go = false;
            while (sp > 0) {
                sp--;
                cur = load_record(copy, column[(size_t)sp * kBlock]);
                slab_range(slab, cur.box, r0, r1);   // (the values that entered it)
                if (PRUNE && r0 > tk)   // t_K has dropped below it since it was pushed
                    continue;
                go = true;
                break;
            }
        }
    }
    if (live) {
        if (SLOTS != kSlotsInMemory) {
#pragma unroll
            for (int i = 0; i < R; i++)
                if (i < k)
                    slots[i] = make_float4(held_t[i], held_u[i], held_v[i], __int_as_float(held_tri[i]));
        }
        if (w.counts)
            w.counts[index] = n;
    }
    if (COUNT)
        add_counters(rc, w.counters);   // (every lane of the wave is here)
}

int check_params(const shray_multihit_params *mp)
{
    if (!mp)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "multihit params are NULL");
    if (mp->struct_size != sizeof(shray_multihit_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_multihit_params.struct_size is %u, this library expects %zu", mp->struct_size,
                    sizeof(shray_multihit_params));
    if (mp->max_hits < 0 || mp->max_hits > SHRAY_MULTIHIT_MAX || mp->max_leaf_tests < 0 || mp->max_leaf_tests > (1 << 24) || mp->reserved != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "multihit params out of range (max_hits %d of 0 .. %d, max_leaf_tests %d, reserved %d)",
                    mp->max_hits, (int)SHRAY_MULTIHIT_MAX, mp->max_leaf_tests, mp->reserved);
    return SHRAY_OK;
}

// the checks every form makes before it touches a scene or a device
int check_query(shray_scene *scene, const shray_multihit_params *mp, const void *rays, int64_t count, const void *hits, const void *counts)
{
    const int rc = check_params(mp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!scene || !rays)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or rays is NULL");
    if (mp->max_hits > 0 && !hits)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "hits is NULL with max_hits %d", mp->max_hits);
    if (mp->max_hits == 0 && !counts)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "nothing is asked for: max_hits is 0 and counts is NULL");
    return SHRAY_OK;
}

template <int SLOTS>
void launch_form(dim3 grid, size_t entries, hipStream_t stream, const SceneView &view, const MultiWork &w)
{
    if (w.counters)
        hipLaunchKernelGGL((all_hits_kernel<SLOTS, false, true>), grid, dim3(kBlock), entries * sizeof(uint32_t), stream, view, w);
    else if (w.counts || w.k == 0)
        hipLaunchKernelGGL((all_hits_kernel<SLOTS, false, false>), grid, dim3(kBlock), entries * sizeof(uint32_t), stream, view, w);
    else
        hipLaunchKernelGGL((all_hits_kernel<SLOTS, true, false>), grid, dim3(kBlock), entries * sizeof(uint32_t), stream, view, w);
}

int trace_device(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(scene, mp, d_rays, count, d_hits, d_counts);
    if (rc)
        return rc;
    const int k = mp->max_hits;
    if (!aligned(d_rays, 16) || (k > 0 && !aligned(d_hits, 16)) || (d_counts && !aligned(d_counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned, the counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))
        return rc;
    MultiWork w{(const float4 *)d_rays, k > 0 ? (float4 *)d_hits : nullptr, d_counts, (uint64_t)count, 0, k, mp->max_leaf_tests, d_counters};
    const size_t entries = (size_t)kBlock * (size_t)(height > 0 ? height : 1);
    return for_each_launch(((uint64_t)count + kBlock - 1) / kBlock, kRaysPerLaunch / kBlock, [&](uint64_t first, dim3 grid) {
        w.first = first * kBlock;
        if (k == 0 || k > 8)
            launch_form<kSlotsInMemory>(grid, entries, stream, q.view, w);
        else if (k == 1)
            launch_form<1>(grid, entries, stream, q.view, w);
        else if (k == 2)
            launch_form<2>(grid, entries, stream, q.view, w);
        else if (k <= 4)
            launch_form<4>(grid, entries, stream, q.view, w);
        else
            launch_form<8>(grid, entries, stream, q.view, w);
        return launched("all-hits ray query");
    });
}

// the blocking forms: the rays to the device, the query on the null stream, the records, counts (and tallies) back
int trace_host(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count, shray_hit *hits,
               int32_t *counts, shray_counters *out)
{
    int rc = check_query(scene, mp, rays, count, hits, counts);
    if (rc)
        return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))   // (the errors of a scene come before any allocation)
        return rc;
    const size_t n = (size_t)count, k = (size_t)mp->max_hits;
    return run_blocking({{rays, n * sizeof(shray_ray)}}, {{hits, n * k * sizeof(shray_hit)}, {counts, counts ? n * sizeof(int32_t) : 0}}, out,
                        [&](DeviceBuffer *d_rays, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return trace_device(scene, mp, d_rays->as<const shray_ray>(), count, d_out[0].as<shray_hit>(),
                                                d_out[1].as<int32_t>(), nullptr, shards);
                        });
}

}   // namespace

static_assert(sizeof(shray_multihit_params) == 16, "shray_multihit_params is 16 bytes");
static_assert(sizeof(shray_ray) == 32 && sizeof(shray_hit) == 16, "the ray query's records");

extern "C" {

void shray_multihit_params_init(shray_multihit_params *mp)
{
    if (!mp)
        return;
    mp->struct_size = sizeof(shray_multihit_params);
    mp->max_hits = 8;
    mp->max_leaf_tests = 10;   // fs:405
    mp->reserved = 0;
}

int shray_trace_all_hits_device(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count,
                                shray_hit *d_hits, int32_t *d_counts, void *hip_stream)
{
    return trace_device(scene, mp, d_rays, count, d_hits, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_all_hits(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count, shray_hit *hits,
                         int32_t *counts)
{
    return trace_host(scene, mp, rays, count, hits, counts, nullptr);
}

int shray_trace_all_hits_counters(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                                  shray_hit *hits, int32_t *counts, shray_counters *out)
{
    if (!out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return trace_host(scene, mp, rays, count, hits, counts, out);
}

}   // extern "C"
