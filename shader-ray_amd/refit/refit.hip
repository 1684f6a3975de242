// refit.hip -- include/shader_ray_refit.h: a resident scene's corners and boxes recomputed in place after its vertices move.
//
// The tree stays; everything the scene derived from coordinates is rewritten with the expressions scene creation used:
// the corners (positions, fp32 and fp16 normals) and the packed triangles (sd_pack_triangles: v0, e0 = v1 - v0, e1 = v0 - v2),
// the node boxes (box3d::add over a node's triangles, vectormath.h:189-195), the literal boxes at the flattener's numbering,
// the box fields of the eight octant copies and of the pair records (packed_layout.h), and exact_div_ok.  The child and link
// words are not touched.  Boxes are built bottom-up by node HEIGHT (a leaf 0, a branch one above its higher child): a node
// of height h reads only boxes of lower heights, and fewer nodes have height h than h - 1 (every one of them has a child of
// height h - 1 of its own), so the wide heights get a launch each -- the launch boundary is the hand-off between workgroups --
// and the narrow rest one workgroup that steps through them behind barriers.  The heights, the order by height and that
// schedule are csrc/tree_order.h's, from the first refit's one readback of octant copy 0.  This library is built apart from
// libshray_hip.so, so the renderer's code objects do not change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "client_internal.h"
#include "device_array_check.h"
#include "error_internal.h"
#include "half_bits.h"
#include "packed_layout.h"
#include "scene_access_internal.h"
#include "shader_ray_refit.h"
#include "tree_order.h"

using namespace shray;

namespace {

constexpr int kBlock = 256;
constexpr int kTailBlock = 1024;          // heights with at most this many branches run in the one-workgroup launch
constexpr float kBumpout = .00001f;       // box3d::add(const vec3 &), vectormath.h:189-195
constexpr double kSahCtrav = 1.0, kSahCisec = 4.0;   // the reference's defaults, bvh.cpp:28-58

struct Box {
    float lo[3], hi[3];
};

// what the kernels report back: the validation pass reads the first 16 bytes, the end of the call all of it
struct RefitFacts {
    int bad_index;            // an index outside [0, vertex_count)
    int non_finite;           // a position or normal that is not finite
    int coords_out_of_range;  // a box coordinate outside exact_div.h's operand ranges
    int unused;
    double weighted_area;     // sum over nodes of area(n) * (SAH_CTRAV, or SAH_CISEC * count for a leaf)
    Box root;
};

// std::min(a, b) and std::max(a, b) as box3d's folds take them (vectormath.h:121-129)
__device__ __forceinline__ float fold_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float fold_max(float a, float b) { return (a < b) ? b : a; }

__global__ void rf_validate(uint64_t items, const float *__restrict__ vertex_data, int stride, int normal_offset, int vertex_count,
                            const int32_t *__restrict__ triangle_vertices, uint64_t corners, RefitFacts *facts)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    if (i < (uint64_t)vertex_count) {
        const float *v = vertex_data + (size_t)stride * i;
        bool finite = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
        if (normal_offset >= 0)
            finite = finite && isfinite(v[normal_offset]) && isfinite(v[normal_offset + 1]) && isfinite(v[normal_offset + 2]);
        if (!finite)
            atomicOr(&facts->non_finite, 1);
    }
    if (triangle_vertices && i < corners) {
        const int32_t index = triangle_vertices[i];
        if (index < 0 || index >= vertex_count)
            atomicOr(&facts->bad_index, 1);
    }
}

// one thread per triangle: its corners (reference layout), normals and packed record, as scene creation makes them
__global__ void rf_corners(uint32_t nt, const float *__restrict__ vertex_data, int stride, int normal_offset,
                           const int32_t *__restrict__ triangle_vertices, float *__restrict__ positions, float *__restrict__ normals32,
                           uint16_t *__restrict__ normals16, PackedTri *__restrict__ tris)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt)
        return;
    float p[9];
    for (int j = 0; j < 3; j++) {
        const size_t corner = 3 * (size_t)t + j;
        const size_t vertex = triangle_vertices ? (size_t)triangle_vertices[corner] : corner;
        const float *v = vertex_data + (size_t)stride * vertex;
        for (int a = 0; a < 3; a++) {
            p[3 * j + a] = v[a];
            positions[3 * corner + a] = v[a];
        }
        if (normal_offset >= 0)
            for (int a = 0; a < 3; a++) {
                const float n = v[normal_offset + a];
                normals32[3 * corner + a] = n;
                normals16[3 * corner + a] = float_to_half_bits(n);      // sd_half_normals
            }
    }
    PackedTri pt;
    for (int a = 0; a < 3; a++) {
        pt.v0[a] = p[a];
        pt.e0[a] = p[3 + a] - p[a];        // e0 = v1 - v0, raytracer.es.fs:304 (sd_pack_triangles)
        pt.e1[a] = p[a] - p[6 + a];        // e1 = v0 - v2, raytracer.es.fs:305
    }
    tris[t] = pt;
}

// one thread per leaf: box3d().add(v - bumpout, v + bumpout) over the corners of its triangles (an empty range keeps the
// initial box, +-FLT_MAX)
__global__ void rf_leaves(uint32_t count, const uint32_t *__restrict__ order, const Topo *__restrict__ topo,
                          const float *__restrict__ positions, Box *__restrict__ boxes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t k = order[i];
    const Topo t = topo[k];
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = FLT_MAX;
        b.hi[a] = -FLT_MAX;
    }
    const size_t end = 9 * ((size_t)t.x + (t.y & ~kLeafFlag));
    for (size_t c = 9 * (size_t)t.x; c < end; c += 3)
        for (int a = 0; a < 3; a++) {
            b.lo[a] = fold_min(b.lo[a], positions[c + a] - kBumpout);
            b.hi[a] = fold_max(b.hi[a], positions[c + a] + kBumpout);
        }
    boxes[k] = b;
}

__device__ __forceinline__ void branch_box(uint32_t k, const Topo *__restrict__ topo, Box *boxes)
{
    const Topo t = topo[k];
    const Box n = boxes[t.x], p = boxes[t.y];
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fold_min(n.lo[a], p.lo[a]);
        b.hi[a] = fold_max(n.hi[a], p.hi[a]);
    }
    boxes[k] = b;
}

// the branches of one height (their children's boxes were written by earlier launches)
__global__ void rf_branches(uint32_t begin, uint32_t count, const uint32_t *__restrict__ order, const Topo *__restrict__ topo,
                            Box *boxes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count)
        branch_box(order[begin + i], topo, boxes);
}

// the remaining heights, narrowest last, in one workgroup: a height's boxes are published to the next by the barrier
// (workgroup scope: every reader and writer is a wave of this workgroup, on one CU)
__global__ void __launch_bounds__(kTailBlock) rf_branches_tail(const uint32_t *__restrict__ height_start, uint32_t first_height,
                                                              uint32_t heights, const uint32_t *__restrict__ order,
                                                              const Topo *__restrict__ topo, Box *boxes)
{
    for (uint32_t h = first_height; h < heights; h++) {
        const uint32_t begin = height_start[h], end = height_start[h + 1];
        for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x)
            branch_box(order[i], topo, boxes);
        __syncthreads();
    }
}

__device__ __forceinline__ double box_area(const Box &b)
{
    const double dx = fmax(0.0, (double)b.hi[0] - (double)b.lo[0]), dy = fmax(0.0, (double)b.hi[1] - (double)b.lo[1]),
                 dz = fmax(0.0, (double)b.hi[2] - (double)b.lo[2]);
    return 2.0 * (dx * dy + dx * dz + dy * dz);
}

__device__ __forceinline__ bool exact_div_operand(float c)
{
    const float m = fabsf(c);
    return c == 0.0f || (m >= 0x1p-70f && m < 0x1p60f);
}

__device__ double block_sum(double v, double *lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (unsigned int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

// one thread per packed node: its box into the literal arrays, the eight octant copies and (a branch) its pair record;
// the operand-range check and the node's SAH term (one partial sum per workgroup, in a fixed order)
__global__ void __launch_bounds__(kBlock) rf_emit(uint32_t n, const Box *__restrict__ boxes, const Topo *__restrict__ topo,
                                                  const int32_t *__restrict__ flat_of_packed, float *__restrict__ boxmin,
                                                  float *__restrict__ boxmax, DeviceNode *__restrict__ copies,
                                                  PackedPair *__restrict__ pairs, RefitFacts *facts, double *__restrict__ partial)
{
    __shared__ double lds[kBlock];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    double term = 0.0;
    if (k < n) {
        const Box b = boxes[k];
        const Topo t = topo[k];
        const size_t g = (size_t)flat_of_packed[k];
        bool in_range = true;
        for (int a = 0; a < 3; a++) {
            boxmin[3 * g + a] = b.lo[a];
            boxmax[3 * g + a] = b.hi[a];
            in_range = in_range && exact_div_operand(b.lo[a]) && exact_div_operand(b.hi[a]);
        }
        if (!in_range)
            atomicOr(&facts->coords_out_of_range, 1);
        // copy o holds the planes a ray of octant o enters and leaves the box by: bit a set, entry = lo (packed_layout.h)
        for (uint32_t o = 0; o < 8; o++) {
            float entry[3], exit[3];
            for (int a = 0; a < 3; a++) {
                const bool positive = (o >> a) & 1u;
                entry[a] = positive ? b.lo[a] : b.hi[a];
                exit[a] = positive ? b.hi[a] : b.lo[a];
            }
            DeviceNode *dn = copies + (size_t)o * n + k;
            *reinterpret_cast<float4 *>(dn->entry_xy) = make_float4(entry[0], entry[1], exit[0], exit[1]);
            *reinterpret_cast<float2 *>(dn->z) = make_float2(entry[2], exit[2]);
        }
        const bool leaf = t.y & kLeafFlag;
        if (!leaf && pairs) {
            const Box neg = boxes[t.x], pos = boxes[t.y];
            PackedPair *pp = pairs + k;
            for (int a = 0; a < 3; a++) {
                pp->lo0[a] = neg.lo[a];
                pp->hi0[a] = neg.hi[a];
                pp->lo1[a] = pos.lo[a];
                pp->hi1[a] = pos.hi[a];
            }
        }
        term = box_area(b) * (leaf ? kSahCisec * (double)(t.y & ~kLeafFlag) : kSahCtrav);
    }
    const double sum = block_sum(term, lds);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(kBlock) rf_finish(uint32_t blocks, const double *__restrict__ partial, const Box *__restrict__ boxes,
                                                    uint32_t root, RefitFacts *facts)
{
    __shared__ double lds[kBlock];
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < blocks; i += blockDim.x)
        v += partial[i];
    const double sum = block_sum(v, lds);
    if (threadIdx.x == 0) {
        facts->weighted_area = sum;
        facts->root = boxes[root];
    }
}

// What the refit keeps per scene (the scene owns it: ShrayRefitScene::state): the nodes ordered by height and their topology
// on the device, the schedule over the heights, and the scratch of the passes.  Built by the first refit from the packed
// tree's child words, which a refit never changes.
struct RefitState {
    TreeOrder levels;         // (its per-node arrays are released once they are on the device)
    DeviceTreeOrder tree;
    DeviceBuffer boxes, partial, facts, staging;
};

// the one readback (octant copy 0), its order by height onto the device, and the scratch
int build_state(const ShrayRefitScene &v, hipStream_t stream, RefitState &st)
{
    const uint32_t n = v.node_count, nt = v.triangle_count;
    std::vector<DeviceNode> copy0(n);
    HIP_TRY(hipMemcpyAsync(copy0.data(), v.packed_nodes, (size_t)n * sizeof(DeviceNode), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const std::string refused = tree_order(copy0.data(), n, v.packed_root << (kNodeShift - kNodeNameShift), nt, 0, kTailBlock, &st.levels);
    if (!refused.empty())
        return fail(SHRAY_ERR_BAD_TREE, "%s", refused.c_str());
    HIP_TRY(st.boxes.grow((size_t)n * sizeof(Box)));
    HIP_TRY(st.partial.grow((size_t)grid_of(n, kBlock) * sizeof(double)));
    HIP_TRY(st.facts.grow(sizeof(RefitFacts)));
    return upload_tree_order(st.levels, st.tree, false, stream);
}

int check_input(const shray_refit_input *in)
{
    if (!in)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "refit input is NULL");
    if (in->struct_size != sizeof(shray_refit_input))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_refit_input.struct_size is %u, this library expects %zu", in->struct_size,
                    sizeof(shray_refit_input));
    if (!in->vertex_data)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "vertex_data is NULL");
    if (in->vertex_count < 0 || in->vertex_stride_floats < 3)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "vertex_count %d, vertex_stride_floats %d (>= 3)", in->vertex_count,
                    in->vertex_stride_floats);
    if (in->normal_offset_floats != -1 &&
        (in->normal_offset_floats < 0 || (int64_t)in->normal_offset_floats + 3 > (int64_t)in->vertex_stride_floats))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "normal_offset_floats %d does not fit a vertex of %d floats (-1: keep the normals)",
                    in->normal_offset_floats, in->vertex_stride_floats);
    return SHRAY_OK;
}

// the scene's refit view, on its device, checked against the input
int scene_of(shray_scene *scene, const shray_refit_input *in, ShrayRefitScene *v)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    int rc = check_input(in);
    if (rc)
        return rc;
    rc = shrayi_scene_refit_view(scene, v);
    if (rc)
        return rc;
    if (!in->triangle_vertices && (uint64_t)in->vertex_count != 3ull * v->triangle_count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%d corners given without triangle_vertices, the scene has %u", in->vertex_count,
                    3u * v->triangle_count);
    if (!v->packed_ok)
        return fail(SHRAY_ERR_BAD_TREE, "the scene has no packed tree (its tables were not proved one canonical tree): it cannot be refit");
    return use_device(v->device);
}

int refit_device(shray_scene *scene, const ShrayRefitScene &v, const shray_refit_input *in, shray_refit_stats *stats, hipStream_t stream)
{
    std::shared_ptr<void> &slot = *v.state;
    if (!slot) {
        auto st = std::make_shared<RefitState>();
        const int rc = build_state(v, stream, *st);
        if (rc)
            return rc;
        slot = st;
    }
    RefitState &st = *static_cast<RefitState *>(slot.get());
    RefitFacts *d_facts = (RefitFacts *)st.facts.p;
    const uint32_t n = v.node_count, nt = v.triangle_count;
    const uint64_t corners = 3ull * nt;
    const int stride = in->vertex_stride_floats, normal_offset = in->normal_offset_floats;

    // 1. validation: nothing of the scene is written before its answer is back
    HIP_TRY(hipMemsetAsync(d_facts, 0, sizeof(RefitFacts), stream));
    const uint64_t items = std::max<uint64_t>((uint64_t)in->vertex_count, in->triangle_vertices ? corners : 0);
    if (items) {
        hipLaunchKernelGGL(rf_validate, dim3(grid_of(items, kBlock)), dim3(kBlock), 0, stream, items, in->vertex_data, stride,
                           normal_offset, in->vertex_count, in->triangle_vertices, corners, d_facts);
        if (const int rc = launched("refit validation"))
            return rc;
    }
    RefitFacts facts;
    HIP_TRY(hipMemcpyAsync(&facts, d_facts, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (facts.bad_index)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "a triangle_vertices entry is outside [0, %d)", in->vertex_count);
    if (facts.non_finite)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "a vertex position or normal is not finite");
    if (const int rc = shrayi_scene_geometry_changed(scene))   // what a later signed-distance query derived is stale now
        return rc;

    // 2. corners, normals, packed triangles
    if (nt)
        hipLaunchKernelGGL(rf_corners, dim3(grid_of(nt, kBlock)), dim3(kBlock), 0, stream, nt, in->vertex_data, stride, normal_offset,
                           in->triangle_vertices, v.positions, v.normals32, v.normals16, (PackedTri *)v.packed_tris);
    // 3. leaf boxes, 4. branch boxes by height
    const uint32_t *order = st.tree.order.as<const uint32_t>();
    const Topo *topo = st.tree.topo.as<const Topo>();
    Box *boxes = (Box *)st.boxes.p;
    for_each_level(
        st.levels,
        [&](uint32_t count) {
            hipLaunchKernelGGL(rf_leaves, dim3(grid_of(count, kBlock)), dim3(kBlock), 0, stream, count, order, topo,
                               (const float *)v.positions, boxes);
            return SHRAY_OK;   // (one check after the last launch, below)
        },
        [&](uint32_t begin, uint32_t count) {
            hipLaunchKernelGGL(rf_branches, dim3(grid_of(count, kBlock)), dim3(kBlock), 0, stream, begin, count, order, topo, boxes);
            return SHRAY_OK;
        },
        [&](uint32_t first_height, uint32_t heights) {
            hipLaunchKernelGGL(rf_branches_tail, dim3(1), dim3(kTailBlock), 0, stream, st.tree.heights.as<const uint32_t>(), first_height,
                               heights, order, topo, boxes);
            return SHRAY_OK;
        });
    // 5. the boxes out, 6. the range check and the SAH cost
    const uint32_t emit_blocks = grid_of(n, kBlock);
    hipLaunchKernelGGL(rf_emit, dim3(emit_blocks), dim3(kBlock), 0, stream, n, (const Box *)boxes, topo, v.flat_of_packed, v.boxmin,
                       v.boxmax, (DeviceNode *)v.packed_nodes, (PackedPair *)v.pair_nodes, d_facts, (double *)st.partial.p);
    hipLaunchKernelGGL(rf_finish, dim3(1), dim3(kBlock), 0, stream, emit_blocks, (const double *)st.partial.p, (const Box *)boxes,
                       v.packed_root, d_facts);
    if (const int rc = launched("refit"))
        return rc;
    // 7. one readback
    HIP_TRY(hipMemcpyAsync(&facts, d_facts, sizeof(facts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t ok = facts.coords_out_of_range ? 0u : 1u;
    if (const int rc = shrayi_scene_set_exact_div_ok(scene, ok))
        return rc;
    if (stats) {
        Box r = facts.root;
        double d[3];
        for (int a = 0; a < 3; a++)
            d[a] = std::max(0.0, (double)r.hi[a] - (double)r.lo[a]);
        const double root_area = 2.0 * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2]);
        stats->sah_cost = root_area > 0.0 ? facts.weighted_area / root_area : 0.0;
        stats->exact_div_ok = (int32_t)ok;
        stats->reserved = 0;
    }
    return SHRAY_OK;
}

}   // namespace

extern "C" {

int shray_scene_refit_device(shray_scene *scene, const shray_refit_input *in, shray_refit_stats *stats, void *hip_stream)
{
    ShrayRefitScene v;
    const int rc = scene_of(scene, in, &v);
    if (rc)
        return rc;
    if (!aligned(in->vertex_data, 4) || !aligned(in->triangle_vertices, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "vertex_data and triangle_vertices must be 4-byte aligned");
    const size_t vertex_bytes = (size_t)in->vertex_count * (size_t)in->vertex_stride_floats * sizeof(float);
    int rc2 = vertex_bytes ? check_device_array(in->vertex_data, vertex_bytes, v.device, "vertex_data", "scene") : SHRAY_OK;
    if (!rc2 && in->triangle_vertices && v.triangle_count)
        rc2 = check_device_array(in->triangle_vertices, 3 * (size_t)v.triangle_count * sizeof(int32_t), v.device, "triangle_vertices", "scene");
    if (rc2)
        return rc2;
    return refit_device(scene, v, in, stats, (hipStream_t)hip_stream);
}

// the host arrays to the device (into the scene's refit staging), then the device form on the null stream
int shray_scene_refit(shray_scene *scene, const shray_refit_input *in, shray_refit_stats *stats)
{
    ShrayRefitScene v;
    int rc = scene_of(scene, in, &v);
    if (rc)
        return rc;
    std::shared_ptr<void> &slot = *v.state;
    if (!slot) {
        auto st = std::make_shared<RefitState>();
        rc = build_state(v, nullptr, *st);
        if (rc)
            return rc;
        slot = st;
    }
    RefitState &st = *static_cast<RefitState *>(slot.get());
    const size_t vertex_bytes = (size_t)in->vertex_count * (size_t)in->vertex_stride_floats * sizeof(float);
    const size_t index_bytes = in->triangle_vertices ? 3 * (size_t)v.triangle_count * sizeof(int32_t) : 0;
    const size_t index_at = (vertex_bytes + 255) & ~(size_t)255;
    HIP_TRY(st.staging.grow(index_at + index_bytes + 16));
    char *base = (char *)st.staging.p;
    if (vertex_bytes)
        HIP_TRY(hipMemcpy(base, in->vertex_data, vertex_bytes, hipMemcpyHostToDevice));
    if (index_bytes)
        HIP_TRY(hipMemcpy(base + index_at, in->triangle_vertices, index_bytes, hipMemcpyHostToDevice));
    shray_refit_input device_in = *in;
    device_in.vertex_data = (const float *)base;
    device_in.triangle_vertices = in->triangle_vertices ? (const int32_t *)(base + index_at) : nullptr;
    return refit_device(scene, v, &device_in, stats, nullptr);
}

int shray_scene_geometry_counts(const shray_scene *scene, int32_t *corners, int32_t *nodes)
{
    ShrayRefitScene v;
    const int rc = shrayi_scene_refit_view(const_cast<shray_scene *>(scene), &v);
    if (rc)
        return rc;
    if (corners)
        *corners = (int32_t)(3u * v.triangle_count);
    if (nodes)
        *nodes = (int32_t)v.node_count;
    return SHRAY_OK;
}

int shray_scene_geometry_download(const shray_scene *scene, float *positions, float *normals, float *boxmin, float *boxmax)
{
    ShrayRefitScene v;
    int rc = shrayi_scene_refit_view(const_cast<shray_scene *>(scene), &v);
    if (rc)
        return rc;
    rc = use_device(v.device);
    if (rc)
        return rc;
    const size_t corner_bytes = 9 * (size_t)v.triangle_count * sizeof(float), node_bytes = 3 * (size_t)v.node_count * sizeof(float);
    if (positions && corner_bytes)
        HIP_TRY(hipMemcpy(positions, v.positions, corner_bytes, hipMemcpyDeviceToHost));
    if (normals && corner_bytes)
        HIP_TRY(hipMemcpy(normals, v.normals32, corner_bytes, hipMemcpyDeviceToHost));
    if (boxmin && node_bytes)
        HIP_TRY(hipMemcpy(boxmin, v.boxmin, node_bytes, hipMemcpyDeviceToHost));
    if (boxmax && node_bytes)
        HIP_TRY(hipMemcpy(boxmax, v.boxmax, node_bytes, hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

}   // extern "C"
