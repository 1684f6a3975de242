// packed_walk.h -- what the one-lane-per-item walks over octant copy 7 of the packed tree share (the closest-point walk,
// point_walk.h, the within-radius walk, near/near.hip, the winding-number walk, winding/winding.hip, the box-overlap walk,
// overlap/overlap.hip, and the all-hits ray walk, multihit/all_hits_walk.h, which multihit/multihit.hip and
// instance_multihit/instance_multihit.hip run): a record's load, the sum over a wave that flushes a walk's work counters, the
// items (points, rays, boxes) of one launch, the readback
// of copy 7 into csrc/tree_order.h's height order, the tree's height and where it is kept per scene, and the refusals of a
// scene before anything is launched.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "client_internal.h"
#include "device_types.h"
#include "error_internal.h"
#include "packed_layout.h"
#include "scene_access_internal.h"
#include "shader_ray_point.h"
#include "tree_order.h"

namespace {

using namespace shray;

constexpr int kBlock = 64;    // one wave per workgroup: a lane's stack column is its own
constexpr int kOctant = 7;    // the copy whose entry planes are boxmin and exit planes boxmax
constexpr uint64_t kPointsPerLaunch = 1ull << 24;   // items (a lane each) of one launch: the grid's threads stay far below 2^32

struct Box {
    float lo[3], hi[3];
};

struct Record {
    Box box;
    uint32_t a, b;
};

__device__ __forceinline__ Record load_record(const char *copy, uint32_t name)
{
    const DeviceNode *n = reinterpret_cast<const DeviceNode *>(copy + ((size_t)name << kNodeNameShift));
    const float4 w0 = *reinterpret_cast<const float4 *>(n);
    const float4 w1 = *(reinterpret_cast<const float4 *>(n) + 1);
    Record r;
    r.box.lo[0] = w0.x;
    r.box.lo[1] = w0.y;
    r.box.hi[0] = w0.z;
    r.box.hi[1] = w0.w;
    r.box.lo[2] = w1.x;
    r.box.hi[2] = w1.y;
    r.a = __float_as_uint(w1.z);
    r.b = __float_as_uint(w1.w);
    return r;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x += __shfl_xor(x, off);
    return x;
}

// The packed tree's topology in height order (tree_order.h), for bottom-up launches whose one workgroup takes the heights
// of at most `tail_width` nodes: a function of the topology only, which a refit does not change.  A blocking readback of
// copy 7; the libraries keep what they need of the result per scene.
inline int packed_tree_order(const ShrayQueryScene &q, uint32_t tail_width, TreeOrder *out)
{
    const uint32_t nodes = q.view.packed_nodes_bytes / (uint32_t)sizeof(DeviceNode);
    std::vector<DeviceNode> host(nodes);
    const char *copy = static_cast<const char *>(q.view.packed_nodes) + (size_t)kOctant * q.view.packed_nodes_bytes;
    HIP_TRY(hipMemcpy(host.data(), copy, q.view.packed_nodes_bytes, hipMemcpyDeviceToHost));
    const std::string refused = tree_order(host.data(), nodes, q.view.packed_root, q.view.triangle_count, kOctant, tail_width, out);
    return refused.empty() ? SHRAY_OK : fail(SHRAY_ERR_BAD_TREE, "%s", refused.c_str());
}

// edges from the root to the deepest leaf of the packed tree
inline int packed_tree_height(const ShrayQueryScene &q, int *height)
{
    TreeOrder t;
    const int rc = packed_tree_order(q, UINT32_MAX, &t);
    if (!rc)
        *height = t.height;
    return rc;
}

// the walk's refusals of a scene before anything is launched: no packed tree, or one deeper than the LDS stack holds
inline int check_walkable(const ShrayQueryScene &q, int height)
{
    if (!q.packed_ok)
        return fail(SHRAY_ERR_BAD_TREE, "the scene has no packed tree (this query walks the packed tree)");
    if (height > SHRAY_POINT_MAX_HEIGHT)
        return fail(SHRAY_ERR_BAD_TREE, "the tree is %d levels deep; the walk's LDS stack holds %d", height, (int)SHRAY_POINT_MAX_HEIGHT);
    return SHRAY_OK;
}

// What the walks keep per scene, in the slot of shrayi_scene_point_state (scene_access_internal.h): the tree's height.  One
// definition, so that every library that shares the slot compiles the same object.
struct PointState {
    int height;
};

// The packed tree's height, read once per scene -- the one synchronisation of a device path, on the scene's first query.
inline int scene_tree_height(const ShrayQueryScene &q, shray_scene *scene, int *height)
{
    std::shared_ptr<void> *slot = nullptr;
    int rc = shrayi_scene_point_state(scene, &slot);
    if (rc)
        return rc;
    if (!*slot) {
        int deepest = 0;
        rc = packed_tree_height(q, &deepest);
        if (rc)
            return rc;
        auto st = std::make_shared<PointState>();
        st->height = deepest;
        *slot = st;
    }
    *height = static_cast<PointState *>(slot->get())->height;
    return SHRAY_OK;
}

// the scene's query view on its device, with the walk's stack height; refused without a packed tree or when too deep
inline int enter_walkable_scene(shray_scene *scene, ShrayQueryScene *q, int *height)
{
    int rc = enter_scene(scene, q);
    if (rc)
        return rc;
    rc = check_walkable(*q, 0);
    if (rc)
        return rc;
    rc = scene_tree_height(*q, scene, height);
    return rc ? rc : check_walkable(*q, *height);
}

}   // namespace
