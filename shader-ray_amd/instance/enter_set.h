// enter_set.h -- how the instanced queries outside libshray_instance.so (instance_multihit/, instance_point/, instance_near/, instance_overlap/, instance_intersect/) enter a set on
// the host.  Host code only; it needs point/packed_walk.h, which libshray_instance.so's own units do not see.
#pragma once

#include "client_internal.h"
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

}   // namespace
