// winding.hip -- include/shader_ray_winding.h: generalized winding numbers on a resident scene by the fast winding number's tree
// walk over per-node dipole expansions, and the winding-signed distance.
//
// The node records are derived once per scene geometry, on the device, on the stream of the query that finds them stale:
// the leaves first, one lane per leaf, then the branches bottom-up by HEIGHT as the refit builds its boxes (refit/refit.hip):
// a branch of height h reads only records of lower heights, so each wide height is a launch of its own and the narrow rest
// one workgroup that steps through them behind barriers.  The order by height, each node's topology and that schedule are
// csrc/tree_order.h's, from one blocking readback of octant copy 7 by the first call (point/packed_walk.h; a refit never
// changes the topology); after that a derivation reads nothing back.  When the records are stale, and the event recorded
// after a derivation that orders it for other streams and for the download, are csrc/client_internal.h's DerivedState.
//
// A query is one lane per point in one-wave workgroups.  The walk's stack holds node names in LDS, level-major, one level per
// edge of the tree's height.  A node costs one 16-byte load of { P, r } for the far-field test; a far node then loads N and M,
// a near branch its child words from copy 7, a near leaf its triangles' corners from the scene's positions (the walk and its
// terms are winding/winding_walk.h's, which libshray_instance_winding.so compiles too).  The winding-signed
// distance runs the closest-point walk (point/point_walk.h, the kernel libshray_point.so runs) and then one lane per point that
// walks for w where the record is a hit.  This library is built apart from libshray_hip.so, so the renderer's code objects do
// not change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>

#include "client_internal.h"
#include "point_walk.h"
#include "shader_ray_winding.h"
#include "trace_common.h"
#include "winding_walk.h"

using namespace shray;

namespace {

constexpr int kDeriveBlock = 256;
constexpr int kTailBlock = 1024;          // heights with at most this many branches run in the one-workgroup launch
constexpr uint64_t kChunk = 1ull << 22;   // points per scratch chunk when the caller keeps no records
constexpr int kF = SHRAY_WINDING_DATA_FLOATS;

// one node's record as the derivation builds it
struct Moments {
    float P[3], r, N[3], A, M[9];
};

// the header's per-triangle terms: N_t, A_t, x_t
__device__ __forceinline__ void triangle_terms(const float *c9, V3 *nt, float *at, V3 *xt)
{
    const V3 a = corner(c9, 0), b = corner(c9, 1), c = corner(c9, 2);
    const V3 n = cross3(b - a, c - a);
    *nt = n * 0.5f;
    *at = 0.5f * sqrtf(dot3(n, n));
    *xt = ((a + b) + c) / 3.0f;
}

// copy 7's box of node k: entry planes lo, exit planes hi
__device__ __forceinline__ void node_box(const DeviceNode *copy7, uint32_t k, float lo[3], float hi[3])
{
    const float4 w0 = *reinterpret_cast<const float4 *>(copy7 + k);
    const float2 w1 = *reinterpret_cast<const float2 *>(copy7[k].z);
    lo[0] = w0.x, lo[1] = w0.y, lo[2] = w1.x;
    hi[0] = w0.z, hi[1] = w0.w, hi[2] = w1.y;
}

// P = S / A, or the box centre when A == 0
__device__ __forceinline__ void set_centre(Moments &m, const float S[3], const float lo[3], const float hi[3])
{
    for (int i = 0; i < 3; i++)
        m.P[i] = m.A == 0.0f ? (lo[i] + hi[i]) * 0.5f : S[i] / m.A;
}

// r = sqrtf of the largest squared distance from P to a corner of the box, corners in the header's order
__device__ __forceinline__ void radius(Moments &m, const float lo[3], const float hi[3])
{
    float e = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const V3 k = mk((c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]);
        const V3 d = k - mk(m.P[0], m.P[1], m.P[2]);
        const float ec = dot3(d, d);
        e = c == 0 ? ec : pick_max(e, ec);
    }
    m.r = sqrtf(e);
}

__device__ __forceinline__ void store(float *data, uint32_t k, const Moments &m)
{
    float4 *o = reinterpret_cast<float4 *>(data + (size_t)kF * k);
    o[0] = make_float4(m.P[0], m.P[1], m.P[2], m.r);
    o[1] = make_float4(m.N[0], m.N[1], m.N[2], m.A);
    o[2] = make_float4(m.M[0], m.M[1], m.M[2], m.M[3]);
    o[3] = make_float4(m.M[4], m.M[5], m.M[6], m.M[7]);
    o[4] = make_float4(m.M[8], 0.0f, 0.0f, 0.0f);
}

__device__ __forceinline__ Moments load(const float *data, uint32_t k)
{
    const float4 *o = reinterpret_cast<const float4 *>(data + (size_t)kF * k);
    const float4 w0 = o[0], w1 = o[1], w2 = o[2], w3 = o[3], w4 = o[4];
    Moments m;
    m.P[0] = w0.x, m.P[1] = w0.y, m.P[2] = w0.z, m.r = w0.w;
    m.N[0] = w1.x, m.N[1] = w1.y, m.N[2] = w1.z, m.A = w1.w;
    m.M[0] = w2.x, m.M[1] = w2.y, m.M[2] = w2.z, m.M[3] = w2.w;
    m.M[4] = w3.x, m.M[5] = w3.y, m.M[6] = w3.z, m.M[7] = w3.w;
    m.M[8] = w4.x;
    return m;
}

// one lane per leaf: the sums over its triangles in index order, P, then M in a second pass
__global__ void __launch_bounds__(kDeriveBlock) wn_leaves(uint32_t count, const uint32_t *__restrict__ order, const Topo *__restrict__ topo,
                                                          const DeviceNode *__restrict__ copy7, const float *__restrict__ positions,
                                                          float *__restrict__ data)
{
    const uint32_t i = blockIdx.x * kDeriveBlock + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t k = order[i];
    const Topo t = topo[k];
    const uint32_t first = t.x, end = t.x + (t.y & ~kLeafFlag);
    Moments m;
    float S[3] = {0.0f, 0.0f, 0.0f};
    m.A = 0.0f;
    for (int j = 0; j < 3; j++)
        m.N[j] = 0.0f;
    for (int j = 0; j < 9; j++)
        m.M[j] = 0.0f;
    for (uint32_t tri = first; tri < end; tri++) {
        V3 nt, xt;
        float at;
        triangle_terms(positions + 9ull * tri, &nt, &at, &xt);
        m.A = m.A + at;
        S[0] = S[0] + xt.x * at, S[1] = S[1] + xt.y * at, S[2] = S[2] + xt.z * at;
        m.N[0] = m.N[0] + nt.x, m.N[1] = m.N[1] + nt.y, m.N[2] = m.N[2] + nt.z;
    }
    float lo[3], hi[3];
    node_box(copy7, k, lo, hi);
    set_centre(m, S, lo, hi);
    for (uint32_t tri = first; tri < end; tri++) {
        V3 nt, xt;
        float at;
        triangle_terms(positions + 9ull * tri, &nt, &at, &xt);
        const float x[3] = {xt.x - m.P[0], xt.y - m.P[1], xt.z - m.P[2]}, n[3] = {nt.x, nt.y, nt.z};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)
                m.M[3 * r + c] = m.M[3 * r + c] + x[r] * n[c];
    }
    radius(m, lo, hi);
    store(data, k, m);
}

// a branch's record from its children's (written by earlier launches, or earlier heights of the tail)
__device__ __forceinline__ void branch_record(uint32_t k, const Topo *__restrict__ topo, const DeviceNode *__restrict__ copy7, float *data)
{
    const Topo t = topo[k];
    const Moments n = load(data, t.x), p = load(data, t.y);
    float lo[3], hi[3];
    node_box(copy7, k, lo, hi);
    Moments m;
    m.A = n.A + p.A;
    const float S[3] = {n.P[0] * n.A + p.P[0] * p.A, n.P[1] * n.A + p.P[1] * p.A, n.P[2] * n.A + p.P[2] * p.A};
    set_centre(m, S, lo, hi);
    for (int j = 0; j < 3; j++)
        m.N[j] = n.N[j] + p.N[j];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            m.M[3 * r + c] = (n.M[3 * r + c] + (n.P[r] - m.P[r]) * n.N[c]) + (p.M[3 * r + c] + (p.P[r] - m.P[r]) * p.N[c]);
    radius(m, lo, hi);
    store(data, k, m);
}

// the branches of one height
__global__ void __launch_bounds__(kDeriveBlock) wn_branches(uint32_t begin, uint32_t count, const uint32_t *__restrict__ order,
                                                            const Topo *__restrict__ topo, const DeviceNode *__restrict__ copy7,
                                                            float *data)
{
    const uint32_t i = blockIdx.x * kDeriveBlock + threadIdx.x;
    if (i < count)
        branch_record(order[begin + i], topo, copy7, data);
}

// the remaining heights in one workgroup: a height's records are published to the next by the barrier (workgroup scope:
// every reader and writer is a wave of this workgroup)
__global__ void __launch_bounds__(kTailBlock) wn_branches_tail(const uint32_t *__restrict__ height_start, uint32_t first_height,
                                                              uint32_t heights, const uint32_t *__restrict__ order,
                                                              const Topo *__restrict__ topo, const DeviceNode *__restrict__ copy7,
                                                              float *data)
{
    for (uint32_t h = first_height; h < heights; h++) {
        const uint32_t begin = height_start[h], end = height_start[h + 1];
        for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x)
            branch_record(order[i], topo, copy7, data);
        __syncthreads();
    }
}

struct PointRange {
    const float4 *points;
    uint64_t count;
    uint64_t first;   // this launch's first point
};

// one lane per point: w, NaN for a point with a non-finite coordinate
__global__ void __launch_bounds__(kBlock) wn_query(WindingView v, PointRange pr, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t wstack[];
    const uint64_t i = pr.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= pr.count)
        return;
    const float4 p = pr.points[i];
    const bool finite = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
    out[i] = finite ? winding_walk(v, mk(p.x, p.y, p.z), wstack + threadIdx.x) : __uint_as_float(0x7fc00000u);
}

// one lane per point after the closest-point walk: the record's distance signed by w (NaN on a miss, no walk)
__global__ void __launch_bounds__(kBlock) wn_signed(WindingView v, PointRange pr, const float4 *__restrict__ records, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t wstack[];
    const uint64_t i = pr.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= pr.count)
        return;
    const float4 r0 = records[2 * i], r1 = records[2 * i + 1];
    if (__float_as_int(r1.z) < 0) {
        out[i] = __uint_as_float(0x7fc00000u);
        return;
    }
    const float4 p = pr.points[i];   // finite: a hit
    const float w = winding_walk(v, mk(p.x, p.y, p.z), wstack + threadIdx.x);
    const float d = sqrtf(r0.w);
    out[i] = (w > 0.5f && r0.w > 0.0f) ? -d : d;
}

// What this library keeps per scene: the topology in height order (from the first call's readback), the node records, and
// when they were derived (DerivedState).
struct WindingState : DerivedState {
    TreeOrder levels;         // (its per-node arrays are released once they are on the device)
    DeviceTreeOrder tree;
    DeviceBuffer data;
};

// the one blocking readback (octant copy 7), its order by height onto the device, and the record buffer
int build_state(const ShrayQueryScene &q, WindingState &st)
{
    int rc = packed_tree_order(q, kTailBlock, &st.levels);
    if (rc || (rc = upload_tree_order(st.levels, st.tree, true, nullptr)))
        return rc;
    HIP_TRY(st.data.alloc((size_t)st.levels.height_start.back() * kF * sizeof(float)));   // (one record per node)
    return SHRAY_OK;
}

// the derivation (file comment), enqueued on `stream`
int derive(const WindingState &st, const SceneView &v, hipStream_t stream)
{
    const DeviceNode *copy7 = reinterpret_cast<const DeviceNode *>(static_cast<const char *>(v.packed_nodes) + (size_t)kOctant * v.packed_nodes_bytes);
    const uint32_t *order = st.tree.order.as<const uint32_t>();
    const Topo *topo = st.tree.topo.as<const Topo>();
    float *data = st.data.as<float>();
    return for_each_level(
        st.levels,
        [&](uint32_t count) {
            hipLaunchKernelGGL(wn_leaves, dim3(grid_of(count, kDeriveBlock)), dim3(kDeriveBlock), 0, stream, count, order, topo, copy7,
                               v.positions, data);
            return launched("winding leaves");
        },
        [&](uint32_t begin, uint32_t count) {
            hipLaunchKernelGGL(wn_branches, dim3(grid_of(count, kDeriveBlock)), dim3(kDeriveBlock), 0, stream, begin, count, order, topo,
                               copy7, data);
            return launched("winding branches");
        },
        [&](uint32_t first_height, uint32_t heights) {
            hipLaunchKernelGGL(wn_branches_tail, dim3(1), dim3(kTailBlock), 0, stream, st.tree.heights.as<const uint32_t>(), first_height,
                               heights, order, topo, copy7, data);
            return launched("winding branches (tail)");
        });
}

// The scene on its device, with this library's state and the records current on `stream` (make_current).  The walk's
// refusals (the point query's) come before anything is launched.
int prepare(shray_scene *scene, ShrayQueryScene *q, WindingState **out, hipStream_t stream)
{
    int rc = enter_scene(scene, q);
    if (rc)
        return rc;
    if ((rc = check_walkable(*q, 0)))
        return rc;
    std::shared_ptr<void> *slot = nullptr;
    uint64_t generation = 0;
    if ((rc = shrayi_scene_winding_state(scene, &slot, &generation)))
        return rc;
    if (!*slot) {
        auto st = std::make_shared<WindingState>();
        if ((rc = build_state(*q, *st)))
            return rc;
        *slot = st;
    }
    WindingState &st = *static_cast<WindingState *>(slot->get());
    if ((rc = check_walkable(*q, st.levels.height)))
        return rc;
    *out = &st;
    return make_current(st, generation, stream, [&] { return derive(st, q->view, stream); });
}

// the checks every query makes before it touches a scene
int check_query(shray_scene *scene, const shray_point *points, int64_t count, float beta, const void *out)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!scene || !points || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, points or out is NULL");
    if (!(beta >= 0.0f))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "beta is %g: it must be >= 0 (+INFINITY: exact)", (double)beta);
    return SHRAY_OK;
}

WindingView view_of(const ShrayQueryScene &q, const WindingState &st, float beta)
{
    return WindingView{st.data.as<const float4>(), static_cast<const char *>(q.view.packed_nodes) + (size_t)kOctant * q.view.packed_nodes_bytes,
                       q.view.positions, q.view.packed_root, beta};
}

int number_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta, float *d_out, hipStream_t stream)
{
    int rc = check_query(scene, d_points, count, beta, d_out);
    if (rc)
        return rc;
    if (!aligned(d_points, 16) || !aligned(d_out, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the point buffer must be 16-byte aligned, the output 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    WindingState *st = nullptr;
    if ((rc = prepare(scene, &q, &st, stream)))
        return rc;
    const WindingView v = view_of(q, *st, beta);
    PointRange pr{(const float4 *)d_points, (uint64_t)count, 0};
    const size_t lds = (size_t)kBlock * (size_t)std::max(st->levels.height, 1) * sizeof(uint32_t);
    return for_each_launch(((uint64_t)count + kBlock - 1) / kBlock, kPointsPerLaunch / kBlock, [&](uint64_t first, dim3 grid) {
        pr.first = first * kBlock;
        hipLaunchKernelGGL(wn_query, grid, dim3(kBlock), lds, stream, v, pr, d_out);
        return launched("winding number");
    });
}

int signed_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta, float *d_signed, shray_closest *d_closest,
                  hipStream_t stream)
{
    int rc = check_query(scene, d_points, count, beta, d_signed);
    if (rc)
        return rc;
    if (!aligned(d_points, 16) || (d_closest && !aligned(d_closest, 16)) || !aligned(d_signed, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "point and record buffers must be 16-byte aligned, the signed values 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    WindingState *st = nullptr;
    if ((rc = prepare(scene, &q, &st, stream)))
        return rc;
    const WindingView v = view_of(q, *st, beta);
    const uint64_t n = (uint64_t)count;
    const size_t lds = (size_t)kBlock * (size_t)std::max(st->levels.height, 1) * sizeof(uint32_t);
    // the closest-point walk, then the sign, a launch's worth of points at a time; without the caller's records, through
    // stream-ordered scratch of at most kChunk records
    const uint64_t chunk = d_closest ? kPointsPerLaunch : std::min(n, kChunk);
    void *scratch = nullptr;
    if (!d_closest)
        HIP_TRY(hipMallocAsync(&scratch, chunk * sizeof(shray_closest), stream));
    for (uint64_t first = 0; first < n && !rc; first += chunk) {
        const uint64_t m = std::min(chunk, n - first);
        shray_closest *records = d_closest ? d_closest + first : (shray_closest *)scratch;
        rc = enqueue_closest(q, st->levels.height, d_points + first, m, records, stream, nullptr);
        if (!rc) {
            const PointRange pr{(const float4 *)(d_points + first), m, 0};
            hipLaunchKernelGGL(wn_signed, dim3(grid_of(m, kBlock)), dim3(kBlock), lds, stream, v, pr, (const float4 *)records,
                               d_signed + first);
            rc = launched("winding-signed distance");
        }
    }
    if (scratch) {
        const hipError_t e = hipFreeAsync(scratch, stream);
        if (!rc)
            HIP_TRY(e);
    }
    return rc;
}

}   // namespace

static_assert(sizeof(Moments) == 17 * sizeof(float), "Moments is the record less its three zeros");

extern "C" {

int shray_winding_number_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta, float *d_out,
                                void *hip_stream)
{
    return number_device(scene, d_points, count, beta, d_out, (hipStream_t)hip_stream);
}

// the points to the device, the device form on the null stream, the values back
int shray_winding_number(shray_scene *scene, const shray_point *points, int64_t count, float beta, float *out)
{
    int rc = check_query(scene, points, count, beta, out);
    if (rc || count == 0)
        return rc;
    ShrayQueryScene q;
    WindingState *st = nullptr;
    if ((rc = prepare(scene, &q, &st, nullptr)))   // (the errors of a scene come before any allocation)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{out, n * sizeof(float)}}, nullptr,
                        [&](DeviceBuffer *d_in, DeviceBuffer *d_out, DeviceCounters *) {
                            return number_device(scene, d_in[0].as<const shray_point>(), count, beta, d_out[0].as<float>(), nullptr);
                        });
}

int shray_winding_signed_distance_device(shray_scene *scene, const shray_point *d_points, int64_t count, float beta,
                                         float *d_signed, shray_closest *d_closest, void *hip_stream)
{
    return signed_device(scene, d_points, count, beta, d_signed, d_closest, (hipStream_t)hip_stream);
}

int shray_winding_signed_distance(shray_scene *scene, const shray_point *points, int64_t count, float beta, float *signed_out,
                                  shray_closest *closest)
{
    int rc = check_query(scene, points, count, beta, signed_out);
    if (rc || count == 0)
        return rc;
    ShrayQueryScene q;
    WindingState *st = nullptr;
    if ((rc = prepare(scene, &q, &st, nullptr)))
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{signed_out, n * sizeof(float)}, {closest, closest ? n * sizeof(shray_closest) : 0}},
                        nullptr, [&](DeviceBuffer *d_in, DeviceBuffer *d_out, DeviceCounters *) {
                            return signed_device(scene, d_in[0].as<const shray_point>(), count, beta, d_out[0].as<float>(),
                                                 d_out[1].as<shray_closest>(), nullptr);
                        });
}

int shray_scene_winding_data_download(shray_scene *scene, float *out)
{
    if (!scene || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or out is NULL");
    ShrayQueryScene q;
    WindingState *st = nullptr;
    const int rc = prepare(scene, &q, &st, nullptr);
    if (rc)
        return rc;
    HIP_TRY(hipEventSynchronize(st->done));   // the derivation may have run on any stream
    HIP_TRY(hipMemcpy(out, st->data.p, st->data.bytes, hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

// Outside the header: for libshray_instance_winding.so.  The scene's node records on its device, current for work enqueued
// on `hip_stream` after the call: prepare()'s one blocking topology readback on the scene's first use, the derivation on that
// stream when the records are stale, and otherwise a wait of that stream for the derivation's event.  Host-only.
int shrayi_scene_winding_records(shray_scene *scene, void *hip_stream, const float **d_records)
{
    if (!scene || !d_records)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or d_records is NULL");
    *d_records = nullptr;
    ShrayQueryScene q;
    WindingState *st = nullptr;
    const int rc = prepare(scene, &q, &st, (hipStream_t)hip_stream);
    if (rc)
        return rc;
    *d_records = st->data.as<const float>();
    return SHRAY_OK;
}

}   // extern "C"
