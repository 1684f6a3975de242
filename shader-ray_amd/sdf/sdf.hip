// sdf.hip -- include/shader_ray_sdf.h: signed distances to a resident scene's surface, the sign from angle-weighted
// pseudonormals.
//
// A query is the closest-point walk (point/point_walk.h: the same kernel libshray_point.so runs, so the records are its
// records) followed by one lane per point that loads the pseudonormal of the record's region and signs the distance.  The
// pseudonormals are derived once per scene geometry, on the device, on the stream of the query that finds them stale:
//   1. per triangle: nhat, the three corner angles, and each corner's position key (-0 made +0);
//   2. the weld: a stable sort of the corners by z, then by (x, y), so that equal positions are adjacent in ascending corner
//      index; a head flag where a position differs from the one before (or either is non-finite), an inclusive scan;
//   3. one lane per vertex (at its head) sums alpha * nhat over its corners, in that order, and writes the sum to each corner;
//   4. the three edge slots of every triangle keyed by their (min, max) vertex, a stable sort, and one lane per edge sums
//      nhat over its slots in ascending slot order and writes the sum to each slot; the topology counts come from the same
//      lanes.
// Every buffer is sized by the triangle count (3T corners, 3T slots), so nothing is read back; the derivation's buffers are
// allocated and freed in stream order, and only the sign data and the counts stay with the scene.  When the sign data is
// stale, and the event recorded after a derivation that orders it for other streams and for the blocking calls, are
// csrc/client_internal.h's DerivedState.  This library is built apart from libshray_hip.so, so the renderer's code objects do
// not change.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <algorithm>
#include <cstring>
#include <memory>

#include "client_internal.h"
#include "point_walk.h"
#include "shader_ray_sdf.h"
#include "trace_common.h"

using namespace shray;

namespace {

constexpr int kSdfBlock = 256;
constexpr uint64_t kChunk = 1ull << 22;   // points per scratch chunk when the caller keeps no records

// the sign data of one triangle (SHRAY_SIGN_DATA_FLOATS): nhat, the vertex pseudonormals of corners a, b, c, the edge
// pseudonormals of AB, AC, BC
constexpr int kFaceAt = 0, kVertexAt = 3, kEdgeAt = 12;

// what surface_info reports, as the derivation's lanes count it
struct SurfaceCounts {
    unsigned long long vertices, edges, boundary, nonmanifold, misoriented, degenerate;
};

// the wave's flags added to one counter with one atomic (every lane of the wave calls it)
__device__ __forceinline__ void count_wave(unsigned long long *counter, bool flag)
{
    const unsigned long long votes = __ballot(flag);
    if ((threadIdx.x & (warpSize - 1)) == 0 && votes)
        atomicAdd(counter, (unsigned long long)__popcll(votes));
}

__device__ __forceinline__ uint32_t key_bits(float x)
{
    const uint32_t b = __float_as_uint(x);
    return b == 0x80000000u ? 0u : b;   // -0 == +0
}

__device__ __forceinline__ bool finite3(const float *v)
{
    return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

// the angle at a corner between the edges u and w leaving it (the header's corner angle)
__device__ __forceinline__ float corner_angle(V3 u, V3 w)
{
    if (dot3(u, u) == 0.0f || dot3(w, w) == 0.0f)
        return 0.0f;
    const V3 x = cross3(u, w);
    return atan_yx(sqrtf(dot3(x, x)), dot3(u, w));
}

// the face normal of the header, and whether it is 0 (the triangle is degenerate)
__device__ __forceinline__ V3 face_normal(const float *c9, bool *degenerate)
{
    const V3 a = mk(c9[0], c9[1], c9[2]), b = mk(c9[3], c9[4], c9[5]), c = mk(c9[6], c9[7], c9[8]);
    const V3 n = cross3(b - a, c - a);
    const float len = sqrtf(dot3(n, n));
    *degenerate = len == 0.0f || !__builtin_isfinite(len);
    return *degenerate ? mk(0.0f, 0.0f, 0.0f) : mk(n.x / len, n.y / len, n.z / len);
}

// 1. per triangle: nhat into the sign data, the corner angles, the corners' position keys and their indices
__global__ void __launch_bounds__(kSdfBlock) sd_triangles(uint32_t nt, const float *__restrict__ positions, float *__restrict__ sign,
                                                          float *__restrict__ alpha, uint32_t *__restrict__ zkey,
                                                          uint64_t *__restrict__ xykey, uint32_t *__restrict__ index,
                                                          SurfaceCounts *counts)
{
    const uint32_t t = blockIdx.x * kSdfBlock + threadIdx.x;
    const bool live = t < nt;
    const float *c9 = positions + 9ull * (live ? t : 0u);   // (nt > 0: a lane past the end reads triangle 0)
    bool degenerate;
    const V3 nh = face_normal(c9, &degenerate);
    count_wave(&counts->degenerate, live && degenerate);
    if (!live)
        return;
    const V3 a = mk(c9[0], c9[1], c9[2]), b = mk(c9[3], c9[4], c9[5]), c = mk(c9[6], c9[7], c9[8]);
    float *s = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * t;
    s[kFaceAt + 0] = nh.x, s[kFaceAt + 1] = nh.y, s[kFaceAt + 2] = nh.z;
    alpha[3ull * t + 0] = corner_angle(b - a, c - a);
    alpha[3ull * t + 1] = corner_angle(c - b, a - b);
    alpha[3ull * t + 2] = corner_angle(a - c, b - c);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const uint64_t k = 3ull * t + j;
        zkey[k] = key_bits(c9[3 * j + 2]);
        xykey[k] = ((uint64_t)key_bits(c9[3 * j]) << 32) | key_bits(c9[3 * j + 1]);
        index[k] = (uint32_t)k;
    }
}

// 2. the (x, y) keys in the order of the z sort
__global__ void __launch_bounds__(kSdfBlock) sd_gather(uint64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ order,
                                                       uint64_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    if (i < n)
        out[i] = key[order[i]];
}

// 2. a vertex starts where the sorted corner's position differs from the one before, or either has a non-finite coordinate
__global__ void __launch_bounds__(kSdfBlock) sd_weld_heads(uint64_t n, const float *__restrict__ positions,
                                                           const uint32_t *__restrict__ order, uint32_t *__restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    if (i >= n)
        return;
    bool starts = i == 0;
    if (!starts) {
        const float *p = positions + 3ull * order[i], *q = positions + 3ull * order[i - 1];
        starts = !finite3(p) || !finite3(q) || !(p[0] == q[0] && p[1] == q[1] && p[2] == q[2]);
    }
    head[i] = starts ? 1u : 0u;
}

// 2. each corner's vertex (0-based) from the scan of the heads
__global__ void __launch_bounds__(kSdfBlock) sd_vertex_of_corner(uint64_t n, const uint32_t *__restrict__ order,
                                                                 const uint32_t *__restrict__ scan, uint32_t *__restrict__ vertex)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    if (i < n)
        vertex[order[i]] = scan[i] - 1u;
}

// 3. one lane per vertex: N_v = sum of alpha_k * nhat_t(k) over its corners in ascending corner index, written to each corner
__global__ void __launch_bounds__(kSdfBlock) sd_vertex_normals(uint64_t n, const uint32_t *__restrict__ order,
                                                               const uint32_t *__restrict__ head, const float *__restrict__ alpha,
                                                               float *__restrict__ sign, SurfaceCounts *counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    const bool starts = i < n && head[i];
    count_wave(&counts->vertices, starts);
    if (!starts)
        return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint64_t j = i;
    do {
        const uint32_t k = order[j];
        const float *nh = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * (k / 3) + kFaceAt;
        const float w = alpha[k];
        sx = sx + w * nh[0];
        sy = sy + w * nh[1];
        sz = sz + w * nh[2];
    } while (++j < n && !head[j]);
    for (uint64_t m = i; m < j; m++) {
        const uint32_t k = order[m];
        float *s = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * (k / 3) + kVertexAt + 3 * (k % 3);
        s[0] = sx, s[1] = sy, s[2] = sz;
    }
}

// 4. the edge slots AB, AC, BC of each triangle: key (min vertex, max vertex) in 2 * bits bits, the slot, and the vertex
// the triangle's traversal (a -> b, c -> a, b -> c) leaves it from
__global__ void __launch_bounds__(kSdfBlock) sd_edge_keys(uint32_t nt, const uint32_t *__restrict__ vertex, int bits,
                                                          uint64_t *__restrict__ key, uint32_t *__restrict__ slot,
                                                          uint32_t *__restrict__ from)
{
    const uint32_t t = blockIdx.x * kSdfBlock + threadIdx.x;
    if (t >= nt)
        return;
    const uint32_t v[3] = {vertex[3ull * t], vertex[3ull * t + 1], vertex[3ull * t + 2]};
    const int ends[3][2] = {{0, 1}, {2, 0}, {1, 2}};   // AB: a -> b, AC: c -> a, BC: b -> c
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t p = v[ends[e][0]], q = v[ends[e][1]];
        const uint64_t s = 3ull * t + e;
        key[s] = ((uint64_t)(p < q ? p : q) << bits) | (p < q ? q : p);
        slot[s] = (uint32_t)s;
        from[s] = p;
    }
}

// 4. one lane per edge: N_e = sum of nhat over its slots in ascending slot order, written to each slot; the edge's counts
__global__ void __launch_bounds__(kSdfBlock) sd_edge_normals(uint64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ order,
                                                             const uint32_t *__restrict__ from, float *__restrict__ sign,
                                                             SurfaceCounts *counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    const bool starts = i < n && (i == 0 || key[i] != key[i - 1]);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint64_t j = i;
    if (starts) {
        do {
            const float *nh = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * (order[j] / 3) + kFaceAt;
            sx = sx + nh[0];
            sy = sy + nh[1];
            sz = sz + nh[2];
        } while (++j < n && key[j] == key[i]);
        for (uint64_t m = i; m < j; m++) {
            const uint32_t s = order[m];
            float *o = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * (s / 3) + kEdgeAt + 3 * (s % 3);
            o[0] = sx, o[1] = sy, o[2] = sz;
        }
    }
    const uint64_t uses = j - i;
    count_wave(&counts->edges, starts);
    count_wave(&counts->boundary, starts && uses == 1);
    count_wave(&counts->nonmanifold, starts && uses >= 3);
    count_wave(&counts->misoriented, starts && uses == 2 && from[order[i]] == from[order[i + 1]]);
}

// the query's second lane per point: the record's pseudonormal, the sign, the signed distance (NaN on a miss)
__global__ void __launch_bounds__(kSdfBlock) sd_sign(uint64_t count, const float4 *__restrict__ points, const float4 *__restrict__ records,
                                                     const float *__restrict__ sign, float *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdfBlock + threadIdx.x;
    if (i >= count)
        return;
    const float4 r0 = records[2 * i], r1 = records[2 * i + 1];
    const int tri = __float_as_int(r1.z), region = __float_as_int(r1.w);
    if (tri < 0) {
        out[i] = __uint_as_float(0x7fc00000u);
        return;
    }
    const float4 p = points[i];
    const int at = region == SHRAY_REGION_FACE ? kFaceAt : region <= SHRAY_REGION_C ? kVertexAt + 3 * region : kEdgeAt + 3 * (region - SHRAY_REGION_AB);
    const float *nrm = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * tri + at;
    const float s = dot3(mk(p.x - r0.x, p.y - r0.y, p.z - r0.z), mk(nrm[0], nrm[1], nrm[2]));
    const float d = sqrtf(r0.w);
    out[i] = (s < 0.0f && r0.w > 0.0f) ? -d : d;
}

// What this library keeps per scene: the tree's height, the sign data and the surface counts, and when they were derived
// (DerivedState).
struct SdfState : DerivedState {
    int height = -1;                 // the packed tree's height, read once (a refit keeps the topology)
    DeviceBuffer sign, counts;
};

int edge_bits(uint64_t corners)
{
    int bits = 1;
    while (bits < 32 && (1ull << bits) < corners)
        bits++;
    return bits;
}

// what a scene with nt triangles keeps: its sign data and the counts
int allocate(SdfState &st, uint32_t nt)
{
    HIP_TRY(st.sign.alloc((size_t)nt * SHRAY_SIGN_DATA_FLOATS * sizeof(float)));
    HIP_TRY(st.counts.alloc(sizeof(SurfaceCounts)));
    return SHRAY_OK;
}

// The derivation's buffers, carved from one stream-ordered allocation: 3T corners or slots of each, and the largest
// temporary storage of the sorts and the scan.  The edge phase reuses the weld's buffers (their contents are dead by then).
struct Scratch {
    float *alpha;
    uint32_t *zkey, *zsorted, *index, *zorder, *order, *head, *scan, *vertex;
    uint64_t *xykey, *xyg, *xys;
    void *temp;
    size_t temp_bytes;
};

int scratch_layout(uint64_t n, char *base, Scratch *sc, size_t *total)
{
    const int bits = edge_bits(n);
    size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, b1, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (size_t)n, 0, 32, nullptr));
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, b2, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (size_t)n, 0, 64, nullptr));
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, b3, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (size_t)n, 0, 2 * bits, nullptr));
    HIP_TRY(rocprim::inclusive_scan(nullptr, b4, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
    sc->temp_bytes = std::max(std::max(b1, b2), std::max(b3, b4));
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + at : nullptr;
        at += (bytes + 255) & ~(size_t)255;
        return p;
    };
    sc->alpha = (float *)take(n * 4);
    for (uint32_t **b : {&sc->zkey, &sc->zsorted, &sc->index, &sc->zorder, &sc->order, &sc->head, &sc->scan, &sc->vertex})
        *b = (uint32_t *)take(n * 4);
    for (uint64_t **b : {&sc->xykey, &sc->xyg, &sc->xys})
        *b = (uint64_t *)take(n * 8);
    sc->temp = take(sc->temp_bytes);
    *total = at;
    return SHRAY_OK;
}

// the kernels, the sorts and the scan of the derivation on `stream`
int derive_into(const Scratch &sc, const SceneView &v, uint64_t n, float *sign, SurfaceCounts *counts, hipStream_t stream)
{
    const uint32_t nt = v.triangle_count;
    size_t bytes = sc.temp_bytes;
    hipLaunchKernelGGL(sd_triangles, dim3(grid_of(nt, kSdfBlock)), dim3(kSdfBlock), 0, stream, nt, v.positions, sign, sc.alpha, sc.zkey, sc.xykey,
                       sc.index, counts);
    if (const int rc = launched("signed-distance triangles"))
        return rc;
    // the weld: z, then (x, y), both stable, so equal positions end adjacent in ascending corner index
    HIP_TRY(rocprim::radix_sort_pairs(sc.temp, bytes, sc.zkey, sc.zsorted, sc.index, sc.zorder, (size_t)n, 0, 32, stream));
    hipLaunchKernelGGL(sd_gather, dim3(grid_of(n, kSdfBlock)), dim3(kSdfBlock), 0, stream, n, (const uint64_t *)sc.xykey, (const uint32_t *)sc.zorder,
                       sc.xyg);
    bytes = sc.temp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(sc.temp, bytes, sc.xyg, sc.xys, sc.zorder, sc.order, (size_t)n, 0, 64, stream));
    hipLaunchKernelGGL(sd_weld_heads, dim3(grid_of(n, kSdfBlock)), dim3(kSdfBlock), 0, stream, n, v.positions, (const uint32_t *)sc.order, sc.head);
    bytes = sc.temp_bytes;
    HIP_TRY(rocprim::inclusive_scan(sc.temp, bytes, sc.head, sc.scan, (size_t)n, rocprim::plus<uint32_t>(), stream));
    hipLaunchKernelGGL(sd_vertex_of_corner, dim3(grid_of(n, kSdfBlock)), dim3(kSdfBlock), 0, stream, n, (const uint32_t *)sc.order,
                       (const uint32_t *)sc.scan, sc.vertex);
    hipLaunchKernelGGL(sd_vertex_normals, dim3(grid_of(n, kSdfBlock)), dim3(kSdfBlock), 0, stream, n, (const uint32_t *)sc.order,
                       (const uint32_t *)sc.head, (const float *)sc.alpha, sign, counts);
    if (const int rc = launched("signed-distance weld"))
        return rc;
    // the edges, in the weld's buffers (its keys are dead now): key, slot and from-vertex per slot, then the stable sort
    const int bits = edge_bits(n);
    hipLaunchKernelGGL(sd_edge_keys, dim3(grid_of(nt, kSdfBlock)), dim3(kSdfBlock), 0, stream, nt, (const uint32_t *)sc.vertex, bits, sc.xykey,
                       sc.index, sc.zkey);
    bytes = sc.temp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(sc.temp, bytes, sc.xykey, sc.xys, sc.index, sc.order, (size_t)n, 0, 2 * bits, stream));
    hipLaunchKernelGGL(sd_edge_normals, dim3(grid_of(n, kSdfBlock)), dim3(kSdfBlock), 0, stream, n, (const uint64_t *)sc.xys, (const uint32_t *)sc.order,
                       (const uint32_t *)sc.zkey, sign, counts);
    return launched("signed-distance edges");
}

// the derivation (file comment), enqueued on `stream` with its scratch allocated and freed in stream order
int derive(SdfState &st, const SceneView &v, hipStream_t stream)
{
    const uint32_t nt = v.triangle_count;
    const uint64_t n = 3ull * nt;
    SurfaceCounts *counts = st.counts.as<SurfaceCounts>();
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(SurfaceCounts), stream));
    if (!nt)
        return SHRAY_OK;
    Scratch sc;
    size_t total = 0;
    int rc = scratch_layout(n, nullptr, &sc, &total);
    if (rc)
        return rc;
    void *base = nullptr;
    HIP_TRY(hipMallocAsync(&base, total, stream));
    scratch_layout(n, (char *)base, &sc, &total);
    rc = derive_into(sc, v, n, st.sign.as<float>(), counts, stream);
    const hipError_t e = hipFreeAsync(base, stream);
    if (rc)
        return rc;
    HIP_TRY(e);
    return SHRAY_OK;
}

// The scene on its device, with this library's state and the sign data current on `stream` (make_current).  With `walk`,
// also the walk's refusals (the point query's) and its stack height.
int prepare(shray_scene *scene, ShrayQueryScene *q, SdfState **out, hipStream_t stream, bool walk)
{
    int rc = enter_scene(scene, q);
    if (rc)
        return rc;
    if (walk && (rc = check_walkable(*q, 0)))
        return rc;
    std::shared_ptr<void> *slot = nullptr;
    uint64_t generation = 0;
    if ((rc = shrayi_scene_sdf_state(scene, &slot, &generation)))
        return rc;
    if (!*slot) {
        auto st = std::make_shared<SdfState>();
        if ((rc = allocate(*st, q->view.triangle_count)))
            return rc;
        *slot = st;
    }
    SdfState &st = *static_cast<SdfState *>(slot->get());
    if (walk) {
        if (st.height < 0 && (rc = packed_tree_height(*q, &st.height)))
            return rc;
        if ((rc = check_walkable(*q, st.height)))
            return rc;
    }
    *out = &st;
    return make_current(st, generation, stream, [&] { return derive(st, q->view, stream); });
}

int signed_device(shray_scene *scene, const shray_point *d_points, int64_t count, float *d_signed, shray_closest *d_closest,
                  hipStream_t stream)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!scene || !d_points || !d_signed)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, points or signed is NULL");
    if (!aligned(d_points, 16) || (d_closest && !aligned(d_closest, 16)) || !aligned(d_signed, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "point and record buffers must be 16-byte aligned, the signed values 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    SdfState *st = nullptr;
    int rc = prepare(scene, &q, &st, stream, true);
    if (rc)
        return rc;
    const uint64_t n = (uint64_t)count;
    const float *sign = st->sign.as<const float>();
    // the walk, then the sign, a launch's worth of points at a time; without the caller's records, through stream-ordered
    // scratch of at most kChunk records
    const uint64_t chunk = d_closest ? kPointsPerLaunch : std::min(n, kChunk);
    void *scratch = nullptr;
    if (!d_closest)
        HIP_TRY(hipMallocAsync(&scratch, chunk * sizeof(shray_closest), stream));
    for (uint64_t first = 0; first < n && !rc; first += chunk) {
        const uint64_t m = std::min(chunk, n - first);
        shray_closest *records = d_closest ? d_closest + first : (shray_closest *)scratch;
        rc = enqueue_closest(q, st->height, d_points + first, m, records, stream, nullptr);
        if (!rc) {
            hipLaunchKernelGGL(sd_sign, dim3(grid_of(m, kSdfBlock)), dim3(kSdfBlock), 0, stream, m, (const float4 *)(d_points + first),
                               (const float4 *)records, sign, d_signed + first);
            rc = launched("signed-distance sign");
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

static_assert(sizeof(shray_surface_info) == 56, "shray_surface_info is 56 bytes");

extern "C" {

int shray_signed_distance_device(shray_scene *scene, const shray_point *d_points, int64_t count, float *d_signed,
                                 shray_closest *d_closest, void *hip_stream)
{
    return signed_device(scene, d_points, count, d_signed, d_closest, (hipStream_t)hip_stream);
}

// the points to the device, the device form on the null stream, the values (and records) back
int shray_signed_distance(shray_scene *scene, const shray_point *points, int64_t count, float *signed_out, shray_closest *closest)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!scene || !points || !signed_out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, points or signed is NULL");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    SdfState *st = nullptr;
    const int rc = prepare(scene, &q, &st, nullptr, true);   // (the errors of a scene come before any allocation)
    if (rc)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{signed_out, n * sizeof(float)}, {closest, closest ? n * sizeof(shray_closest) : 0}},
                        nullptr, [&](DeviceBuffer *d_in, DeviceBuffer *d_out, DeviceCounters *) {
                            return signed_device(scene, d_in[0].as<const shray_point>(), count, d_out[0].as<float>(),
                                                 d_out[1].as<shray_closest>(), nullptr);
                        });
}

int shray_scene_surface_info(shray_scene *scene, shray_surface_info *info)
{
    if (!scene || !info)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or info is NULL");
    ShrayQueryScene q;
    SdfState *st = nullptr;
    const int rc = prepare(scene, &q, &st, nullptr, false);
    if (rc)
        return rc;
    HIP_TRY(hipEventSynchronize(st->done));   // the derivation may have run on any stream
    SurfaceCounts c;
    HIP_TRY(hipMemcpy(&c, st->counts.p, sizeof(c), hipMemcpyDeviceToHost));
    memset(info, 0, sizeof(*info));
    info->vertices = (int64_t)c.vertices;
    info->edges = (int64_t)c.edges;
    info->boundary_edges = (int64_t)c.boundary;
    info->nonmanifold_edges = (int64_t)c.nonmanifold;
    info->misoriented_edges = (int64_t)c.misoriented;
    info->degenerate_triangles = (int64_t)c.degenerate;
    info->closed = (c.boundary == 0 && c.nonmanifold == 0 && c.misoriented == 0) ? 1 : 0;
    return SHRAY_OK;
}

int shray_scene_sign_data_download(shray_scene *scene, float *out)
{
    if (!scene || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or out is NULL");
    ShrayQueryScene q;
    SdfState *st = nullptr;
    const int rc = prepare(scene, &q, &st, nullptr, false);
    if (rc)
        return rc;
    HIP_TRY(hipEventSynchronize(st->done));   // the derivation may have run on any stream
    if (q.view.triangle_count)
        HIP_TRY(hipMemcpy(out, st->sign.p, (size_t)q.view.triangle_count * SHRAY_SIGN_DATA_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

// Not in the header: for libshray_instance_sdf.so, which signs in a member scene's object space.  The scene's sign data
// (SHRAY_SIGN_DATA_FLOATS floats per triangle, device memory of the scene's device) current for work enqueued on
// `hip_stream` after this call: derived there when it is stale (first use, or after a refit), else that stream waits for the
// derivation's event.  The pointer stays the scene's own until it is destroyed; a re-derivation rewrites it in place.
// Host-only; makes the scene's device current and waits for nothing.
int shrayi_scene_sign_data(shray_scene *scene, void *hip_stream, const float **d_sign)
{
    if (!scene || !d_sign)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or d_sign is NULL");
    *d_sign = nullptr;
    ShrayQueryScene q;
    SdfState *st = nullptr;
    const int rc = prepare(scene, &q, &st, (hipStream_t)hip_stream, false);
    if (rc)
        return rc;
    *d_sign = st->sign.as<const float>();
    return SHRAY_OK;
}

}   // extern "C"
