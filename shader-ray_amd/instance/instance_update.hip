// instance_update.hip -- the device update of an instance set (shray_instance_set_update_device): the host update's set,
// built on the set's device and stream-ordered.  One pass per instance runs
// invert and place_box, the host's own functions, and sets the refusal word; the ids are then sorted once per axis by
// (centre[axis], id), and the top level is built level by level from the three sorted lists: a segment's centroid extent on
// axis c is its last minus its first entry in list c, its left child takes the first count / 2 entries of the chosen axis's
// list, and the other two lists are partitioned stably by that flag, so every list stays in (key, id) order within each
// segment and each split is the set std::nth_element leaves on either side of the median.  Node positions are the host's
// pre-order allocation, a function of the counts alone (segment_at).  Boxes are folded bottom-up in float: the outward
// roundings are monotone, so the fold of the rounded leaf boxes is the rounding of the host's double fold.  Everything goes
// to scratch first; the last kernel copies it over the set's arrays unless an instance was refused.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "device_array_check.h"
#include "error_internal.h"
#include "scene_access_internal.h"
#include "set_internal.h"

using namespace shray;
using namespace shray_set;

namespace {

constexpr int kUpdateBlock = 256;
constexpr int32_t kNoRefusal = 0x7f7f7f7f;   // the refusal word before the pass (a byte memset): above every instance index

// where sorted position p sits after `depth` levels of splits: the segment [first, first + count), its node, and (count >= 2)
// the position of its children's pair.  A node's left child holds count / 2 instances; its pair follows the parent's pair,
// and the right child's pair follows the left child's subtree of 2 * (count / 2) - 1 nodes (the host's pre-order allocation).
struct Segment {
    uint32_t first, count, node, pair;
};

__device__ __forceinline__ Segment segment_at(uint32_t p, uint32_t n, int depth)
{
    Segment g{0u, n, 0u, 1u};
    for (int d = 0; d < depth && g.count >= 2u; ++d) {
        const uint32_t half = g.count / 2u;
        if (p < g.first + half)
            g = Segment{g.first, half, g.pair, g.pair + 2u};
        else
            g = Segment{g.first + half, g.count - half, g.pair + 1u, g.pair + 2u * half};
    }
    return g;
}

// an unsigned key in the order of the doubles, -0 with +0 (c + 0.0 is +0 for either zero)
__device__ __forceinline__ uint64_t centre_key(double c)
{
    const uint64_t u = (uint64_t)__double_as_longlong(c + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ bool refused_already(const int32_t *refused) { return *refused != kNoRefusal; }

__global__ void __launch_bounds__(kUpdateBlock) iu_iota(uint32_t n, uint32_t *ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        ids[i] = i;
}

// one thread per instance: W, the leaf node, the centre and its keys; a refused transform lowers the refusal word
__global__ void __launch_bounds__(kUpdateBlock) iu_instances(uint32_t n, const float *__restrict__ object_to_world,
                                                             const float4 *__restrict__ live_records, const SceneView *__restrict__ views,
                                                             float4 *__restrict__ records, TopNode *__restrict__ leaves,
                                                             double *__restrict__ centres, uint64_t *__restrict__ keys, int32_t *refused)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float m[12], w[12];
    for (int j = 0; j < 12; ++j)
        m[j] = object_to_world[12 * (size_t)i + j];
    double condition = 0.0;
    if (!invert(m, w, &condition)) {
        atomicMin(refused, (int32_t)i);
        return;
    }
    const uint32_t slot = __float_as_uint(live_records[4 * (size_t)i + 3].x);   // (a set's scene slots never change)
    const SceneView &v = views[slot];
    const size_t root = 3u * (size_t)v.tree_root;
    const float rb[6] = {v.boxmin[root], v.boxmin[root + 1], v.boxmin[root + 2], v.boxmax[root], v.boxmax[root + 1], v.boxmax[root + 2]};
    BoxRef b;
    place_box(m, rb, condition, b);
    for (int r = 0; r < 3; ++r)
        records[4 * (size_t)i + r] = make_float4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    records[4 * (size_t)i + 3] = make_float4(__uint_as_float(slot), 0.0f, 0.0f, 0.0f);
    TopNode leaf;
    for (int c = 0; c < 3; ++c) {
        leaf.lo[c] = round_down(b.lo[c]);
        leaf.hi[c] = round_up(b.hi[c]);
        centres[(size_t)c * n + i] = b.centre[c];
        keys[(size_t)c * n + i] = centre_key(b.centre[c]);
    }
    leaf.k = round_up(b.k);
    leaf.link = kLeafBit | i;
    leaves[i] = leaf;
}

// level `depth`, one thread per sorted position: the split axis of the position's segment (the host's: the longest centroid
// extent, the lowest axis on a tie), its left-half flag by instance, and the node's link
__global__ void __launch_bounds__(kUpdateBlock) iu_split(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                         const double *__restrict__ centres, uint32_t *__restrict__ left_of,
                                                         TopNode *__restrict__ nodes, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    if (g.count < 2u)
        return;
    const uint32_t last = g.first + g.count - 1u;
    double extent[3];
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)c * n;
        extent[c] = centres[at + lists[at + last]] - centres[at + lists[at + g.first]];
    }
    int axis = 0;
    for (int c = 1; c < 3; ++c)
        if (extent[c] > extent[axis])
            axis = c;
    left_of[lists[(size_t)axis * n + p]] = p - g.first < g.count / 2u ? 1u : 0u;
    if (p == g.first)
        nodes[g.node].link = (uint32_t)axis << 29 | g.pair;
}

// every list's left-half flags by position (0 in segments that no longer split)
__global__ void __launch_bounds__(kUpdateBlock) iu_flags(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                         const uint32_t *__restrict__ left_of, uint32_t *__restrict__ flags,
                                                         const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const bool splits = segment_at(p, n, depth).count >= 2u;
    for (int c = 0; c < 3; ++c)
        flags[(size_t)c * n + p] = splits ? left_of[lists[(size_t)c * n + p]] : 0u;
}

// the stable partition of every list within each splitting segment: the left half first, each half in its old order
__global__ void __launch_bounds__(kUpdateBlock) iu_scatter(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                           const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offsets,
                                                           uint32_t *__restrict__ out, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)c * n;
        const uint32_t id = lists[at + p];
        if (g.count < 2u) {
            out[at + p] = id;
            continue;
        }
        const uint32_t before = offsets[at + p] - offsets[at + g.first];   // left entries in [first, p)
        out[at + (flags[at + p] ? g.first + before : g.first + g.count / 2u + (p - g.first - before))] = id;
    }
}

// after the last level every segment is one instance: its leaf node
__global__ void __launch_bounds__(kUpdateBlock) iu_leaves(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                          const TopNode *__restrict__ leaves, TopNode *__restrict__ nodes,
                                                          const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    nodes[segment_at(p, n, depth).node] = leaves[lists[p]];
}

// level `depth`'s branches from their children's boxes (min / max are exact; the link was written by iu_split)
__global__ void __launch_bounds__(kUpdateBlock) iu_fold(uint32_t n, int depth, TopNode *nodes, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    if (g.count < 2u || p != g.first)
        return;
    const TopNode a = nodes[g.pair], b = nodes[g.pair + 1u];
    TopNode t;
    for (int c = 0; c < 3; ++c) {
        t.lo[c] = (b.lo[c] < a.lo[c]) ? b.lo[c] : a.lo[c];
        t.hi[c] = (a.hi[c] < b.hi[c]) ? b.hi[c] : a.hi[c];
    }
    t.k = (a.k < b.k) ? b.k : a.k;
    t.link = nodes[g.node].link;
    nodes[g.node] = t;
}

// the scratch over the set's arrays, or nothing when an instance was refused; the outcome into the status word
__global__ void __launch_bounds__(kUpdateBlock) iu_commit(uint32_t n, const TopNode *__restrict__ new_nodes,
                                                          const float4 *__restrict__ new_records, const float *__restrict__ new_transforms,
                                                          const uint32_t *__restrict__ new_views, uint32_t view_words, TopNode *__restrict__ nodes,
                                                          float4 *__restrict__ records, float *__restrict__ transforms,
                                                          uint32_t *__restrict__ views, const int32_t *refused, int32_t *status)
{
    const int32_t r = *refused;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (first == 0)
        *status = r == kNoRefusal ? -1 : r;
    if (r != kNoRefusal)
        return;
    for (size_t k = first; k < 2 * (size_t)n - 1; k += stride)
        nodes[k] = new_nodes[k];
    for (size_t k = first; k < 4 * (size_t)n; k += stride)
        records[k] = new_records[k];
    if (new_transforms)
        for (size_t k = first; k < 12 * (size_t)n; k += stride)
            transforms[k] = new_transforms[k];
    for (size_t k = first; k < view_words; k += stride)
        views[k] = new_views[k];
}

// ---- the device update's host side -------------------------------------------------------------------------------------------

unsigned int blocks_of(size_t items) { return (unsigned int)((items + kUpdateBlock - 1) / kUpdateBlock); }

// the scratch of the device update, made once per set on its device; the ids are written on `stream`
int make_update(shray_instance_set *set, hipStream_t stream, std::unique_ptr<DeviceUpdate> &out)
{
    auto u = std::make_unique<DeviceUpdate>();
    const uint32_t n = (uint32_t)set->scenes.size();
    u->n = n;
    while ((1u << u->depth) < n)
        u->depth++;
    for (shray_scene *s : set->scenes)
        if (std::find(u->distinct.begin(), u->distinct.end(), s) == u->distinct.end())
            u->distinct.push_back(s);
    const size_t m = 3 * (size_t)n;
    HIP_TRY(u->words.alloc(2 * sizeof(int32_t)));
    HIP_TRY(u->records.alloc(4 * (size_t)n * sizeof(float4)));
    HIP_TRY(u->leaves.alloc((size_t)n * sizeof(TopNode)));
    HIP_TRY(u->nodes.alloc((2 * (size_t)n - 1) * sizeof(TopNode)));
    HIP_TRY(u->centres.alloc(m * sizeof(double)));
    HIP_TRY(u->keys.alloc(m * sizeof(uint64_t)));
    HIP_TRY(u->sorted_keys.alloc(m * sizeof(uint64_t)));
    HIP_TRY(u->ids.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(u->lists[0].alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->lists[1].alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->left_of.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(u->flags.alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->offsets.alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->views.alloc(u->distinct.size() * sizeof(SceneView)));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)n, 0, 64, stream));
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, m,
                                    rocprim::plus<uint32_t>(), stream));
    u->temp_bytes = std::max(sort_bytes, scan_bytes);
    HIP_TRY(u->temp.alloc(u->temp_bytes));
    HIP_TRY(hipEventCreateWithFlags(&u->finished, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(u->words.p, 0xff, 2 * sizeof(int32_t), stream));   // status -1: no update refused yet
    hipLaunchKernelGGL(iu_iota, dim3(blocks_of(n)), dim3(kUpdateBlock), 0, stream, n, u->ids.as<uint32_t>());
    if (const int rc = launched("instance update set-up"))
        return rc;
    out = std::move(u);
    return SHRAY_OK;
}

int update_device(shray_instance_set *set, const float *d_object_to_world, hipStream_t stream)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    const uint32_t n = (uint32_t)set->scenes.size();
    if (d_object_to_world) {
        if (!aligned(d_object_to_world, 4))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "object_to_world must be 4-byte aligned");
        rc = check_device_array(d_object_to_world, 12 * (size_t)n * sizeof(float), set->host.device, "object_to_world", "set");
        if (rc)
            return rc;
    }
    if (!set->update) {
        rc = make_update(set, stream, set->update);
        if (rc)
            return rc;
    }
    DeviceUpdate &u = *set->update;
    // the member views as they are now (a refit may have flipped exact_div_ok), uploaded when they changed
    std::vector<SceneView> views(u.distinct.size());
    for (size_t k = 0; k < views.size(); ++k) {
        ShrayQueryScene q;
        rc = shrayi_scene_query_view(u.distinct[k], &q);
        if (rc)
            return rc;
        views[k] = q.view;
    }
    const size_t view_bytes = views.size() * sizeof(SceneView);
    if (!u.views_staged || memcmp(views.data(), u.staged.data(), view_bytes) != 0) {
        rc = stage(u.staging, stream, u.views.p, views.data(), view_bytes);
        if (rc)
            return rc;
        u.staged = views;
        u.views_staged = true;
    }
    if ((rc = current_maps(set, stream)))
        return rc;
    const DeviceBuffer &transforms = set->maps->transforms;
    int32_t *refused = u.words.as<int32_t>();
    const size_t m = 3 * (size_t)n;
    const dim3 grid(blocks_of(n)), block(kUpdateBlock);
    HIP_TRY(hipMemsetAsync(refused, 0x7f, sizeof(int32_t), stream));   // kNoRefusal
    // 1. one pass per instance
    hipLaunchKernelGGL(iu_instances, grid, block, 0, stream, n, d_object_to_world ? d_object_to_world : transforms.as<const float>(),
                       (const float4 *)set->dev.records, u.views.as<const SceneView>(), u.records.as<float4>(), u.leaves.as<TopNode>(),
                       u.centres.as<double>(), u.keys.as<uint64_t>(), refused);
    if ((rc = launched("instance update")))
        return rc;
    // 2. the ids by (centre[c], id), once per axis
    uint32_t *lists = u.lists[0].as<uint32_t>(), *spare = u.lists[1].as<uint32_t>();
    for (int c = 0; c < 3; ++c) {
        size_t bytes = u.temp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(u.temp.p, bytes, u.keys.as<const uint64_t>() + (size_t)c * n, u.sorted_keys.as<uint64_t>() + (size_t)c * n,
                                          u.ids.as<const uint32_t>(), lists + (size_t)c * n, (size_t)n, 0, 64, stream));
    }
    // 3. the levels, top-down
    for (int d = 0; d < u.depth; ++d) {
        hipLaunchKernelGGL(iu_split, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.centres.as<const double>(),
                           u.left_of.as<uint32_t>(), u.nodes.as<TopNode>(), (const int32_t *)refused);
        hipLaunchKernelGGL(iu_flags, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.left_of.as<const uint32_t>(),
                           u.flags.as<uint32_t>(), (const int32_t *)refused);
        size_t bytes = u.temp_bytes;
        HIP_TRY(rocprim::exclusive_scan(u.temp.p, bytes, u.flags.as<const uint32_t>(), u.offsets.as<uint32_t>(), 0u, m,
                                        rocprim::plus<uint32_t>(), stream));
        hipLaunchKernelGGL(iu_scatter, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.flags.as<const uint32_t>(),
                           u.offsets.as<const uint32_t>(), spare, (const int32_t *)refused);
        std::swap(lists, spare);
    }
    // 4. the leaves, then the boxes bottom-up
    hipLaunchKernelGGL(iu_leaves, grid, block, 0, stream, n, u.depth, (const uint32_t *)lists, u.leaves.as<const TopNode>(),
                       u.nodes.as<TopNode>(), (const int32_t *)refused);
    for (int d = u.depth - 1; d >= 0; --d)
        hipLaunchKernelGGL(iu_fold, grid, block, 0, stream, n, d, u.nodes.as<TopNode>(), (const int32_t *)refused);
    // 5. the commit
    const uint32_t view_words = (uint32_t)(view_bytes / sizeof(uint32_t));
    hipLaunchKernelGGL(iu_commit, dim3(std::min(blocks_of(12 * (size_t)n), 1024u)), block, 0, stream, n, u.nodes.as<const TopNode>(),
                       u.records.as<const float4>(), d_object_to_world, u.views.as<const uint32_t>(), view_words, set->dev.nodes,
                       set->dev.records, d_object_to_world ? transforms.as<float>() : nullptr, (uint32_t *)set->dev.views,
                       (const int32_t *)refused, refused + 1);
    if ((rc = launched("instance update")))
        return rc;
    HIP_TRY(hipEventRecord(u.finished, stream));
    u.enqueued = true;
    set->host_stale = true;
    return SHRAY_OK;
}

}   // namespace

extern "C" {

int shray_instance_set_update_device(shray_instance_set *set, const float *d_object_to_world, void *hip_stream)
{
    return update_device(set, d_object_to_world, (hipStream_t)hip_stream);
}

int shray_instance_set_update_status(shray_instance_set *set, int32_t *refused)
{
    if (!set || !refused)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or refused is NULL");
    *refused = -1;
    if (!set->update || !set->update->enqueued)
        return SHRAY_OK;
    const int rc = use_device(set->host.device);
    if (rc)
        return rc;
    HIP_TRY(hipEventSynchronize(set->update->finished));
    HIP_TRY(hipMemcpy(refused, set->update->words.as<int32_t>() + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

}   // extern "C"
