// enter_set.h -- how the instanced queries outside libshray_instance.so (instance_multihit/, instance_point/, instance_near/,
// instance_overlap/, instance_intersect/) enter a set on the host, and what their device forms do between their refusals and
// their launches, beside point/first_k_query.h's scaffold: a library keeps its kernel, its Work struct, its nouns and its
// launch ladder.  Host code only; it needs point/packed_walk.h and point/first_k_query.h, which libshray_instance.so's own
// units, built without -Ipoint, do not see.
#pragma once

#include "client_internal.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "top_level.h"

namespace {

// the set's arrays on its device, and the height of its tallest member tree (each member's read back once per scene)
inline int enter_set(shray_instance_set *set, ShrayInstanceSetDevice *d, int *height)
{
    int rc = shrayi_instance_set_device_arrays(set, d);
    if (rc)
        return rc;
    if ((rc = use_device(d->device)))
        return rc;
    *height = 0;
    for (int32_t s = 0; s < d->scene_count; s++) {
        ShrayQueryScene q;
        int h = 0;
        if ((rc = shrayi_scene_query_view(d->scenes[s], &q)) || (rc = check_walkable(q, 0)) || (rc = scene_tree_height(q, d->scenes[s], &h)) ||
            (rc = check_walkable(q, h)))
            return rc;
        *height = h > *height ? h : *height;
    }
    return SHRAY_OK;
}

// the entry alone: a blocking form's, whose set's errors come before any allocation
inline int enter_set(shray_instance_set *set)
{
    ShrayInstanceSetDevice d;
    int height = 0;
    return enter_set(set, &d, &height);
}

// an entered set as a kernel's launch takes it
struct SetWalk {
    const TopNode *nodes;
    const float4 *records;
    const float4 *maps;       // the forward maps' rows, three per instance; nullptr for a walk that does not ask for them
    const SceneView *views;
    int levels;               // a lane's stack column: the tallest member scene's height, at least 1
    int32_t *instances;       // k per item: the caller's, or scratch, or nullptr

    // a workgroup's LDS: the lanes' columns of `entry`-byte entries, then the wave's top-level stack
    size_t lds(size_t entry) const { return (size_t)kBlock * (size_t)levels * entry + kTopStack * sizeof(uint32_t); }
};

// A device form over a set, after its refusals: the set entered, its forward maps current on `stream` (with_maps), and
// launches(walk), which returns the form's code.  The kernel instance that keeps its K best in an item's output slots
// keeps the instance part of its keys beside them: without an instance buffer of the caller's, in scratch that is taken
// and given back in stream order around the launches.
template <typename Launches>
int walk_set(shray_instance_set *set, bool with_maps, int k, int64_t count, int32_t *d_instances, hipStream_t stream, Launches &&launches)
{
    ShrayInstanceSetDevice d;
    int height = 0;
    int rc = enter_set(set, &d, &height);
    if (rc)
        return rc;
    const float *d_maps = nullptr;
    if (with_maps && (rc = shrayi_instance_set_forward_maps(set, stream, &d_maps)))
        return rc;
    int32_t *scratch = nullptr;
    if (kept_in_memory(k) && !d_instances) {
        HIP_TRY(hipMallocAsync((void **)&scratch, (size_t)count * (size_t)k * sizeof(int32_t), stream));
        d_instances = scratch;
    }
    rc = launches(SetWalk{static_cast<const TopNode *>(d.nodes), static_cast<const float4 *>(d.records),
                          reinterpret_cast<const float4 *>(d_maps), static_cast<const SceneView *>(d.views), (int)stack_levels(height),
                          d_instances});
    if (scratch) {
        const hipError_t e = hipFreeAsync(scratch, stream);
        if (e != hipSuccess && !rc)
            rc = fail(SHRAY_ERR_DEVICE, "hipFreeAsync failed: %s", hipGetErrorString(e));
    }
    return rc;
}

}   // namespace
