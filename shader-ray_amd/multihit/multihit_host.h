// multihit_host.h -- what the hosts of the two all-hits ray queries share (multihit.hip, and the instanced form,
// instance_multihit/instance_multihit.hip): the check of a shray_multihit_params and the rays' nouns.  Host-only, internal to
// the libraries.
#pragma once

#include "error_internal.h"
#include "first_k_query.h"
#include "shader_ray_multihit.h"

namespace {

inline int check_params(const shray_multihit_params *mp)
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

// the checks every form makes before it touches a scene, a set or a device
inline int check_query(const Nouns &n, const void *owner, const shray_multihit_params *mp, const void *rays, int64_t count, const void *hits,
                       const void *counts)
{
    const int rc = check_params(mp);
    return rc ? rc : check_first_k(n, owner, rays, count, mp->max_hits, hits, counts);
}

static_assert(sizeof(shray_multihit_params) == 16, "shray_multihit_params is 16 bytes");
static_assert(sizeof(shray_ray) == 32 && sizeof(shray_hit) == 16, "the ray query's records");

}   // namespace
