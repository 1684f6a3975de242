// params_check.h -- the params refusals of include/shader_ray_overlap.h, include/shader_ray_intersect.h and
// include/shader_ray_clearance.h, each made by the query's library (overlap/overlap.hip, intersect/intersect.hip,
// clearance/clearance.hip) and by its instanced form (instance_overlap/, instance_intersect/, instance_clearance/): the struct itself, then the misuse of the ANY flag, which a library makes at its own place among its
// refusals.  Host code only.
#pragma once

#include "client_internal.h"
#include "shader_ray_clearance.h"
#include "shader_ray_intersect.h"
#include "shader_ray_overlap.h"

namespace {

inline int check_params(const shray_overlap_params *op)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params are NULL");
    if (op->struct_size != sizeof(shray_overlap_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_overlap_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_overlap_params));
    if (op->max_triangles < 0 || op->max_triangles > SHRAY_OVERLAP_MAX || (op->flags & ~(uint32_t)SHRAY_OVERLAP_ANY) || op->reserved != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "overlap params out of range (max_triangles %d of 0 .. %d, flags 0x%x, reserved %d)",
                    op->max_triangles, (int)SHRAY_OVERLAP_MAX, op->flags, op->reserved);
    return SHRAY_OK;
}

inline int check_any(const shray_overlap_params *op, const void *counts)
{
    if ((op->flags & SHRAY_OVERLAP_ANY) && (op->max_triangles != 0 || !counts))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_OVERLAP_ANY needs max_triangles 0 (it is %d) and counts", op->max_triangles);
    return SHRAY_OK;
}

// `known`: the flags of the form that asks (only the instance form knows SHRAY_INTERSECT_SKIP_OWN_INSTANCE)
inline int check_params(const shray_intersect_params *op, uint32_t known)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "intersect params are NULL");
    if (op->struct_size != sizeof(shray_intersect_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_intersect_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_intersect_params));
    if (op->max_triangles < 0 || op->max_triangles > SHRAY_INTERSECT_MAX || (op->flags & ~known) || op->reserved != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "intersect params out of range (max_triangles %d of 0 .. %d, flags 0x%x, reserved %d)",
                    op->max_triangles, (int)SHRAY_INTERSECT_MAX, op->flags, op->reserved);
    return SHRAY_OK;
}

inline int check_any(const shray_intersect_params *op, const void *counts)
{
    if ((op->flags & SHRAY_INTERSECT_ANY) && (op->max_triangles != 0 || !counts))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_INTERSECT_ANY needs max_triangles 0 (it is %d) and counts", op->max_triangles);
    return SHRAY_OK;
}

// (max_dist2 is not refused: a NaN or a negative one is a query that is not walked)
// `known`: the flags of the form that asks (only instance_clearance/'s instance form knows SHRAY_CLEARANCE_SKIP_OWN_INSTANCE)
inline int check_params(const shray_clearance_params *op, uint32_t known = SHRAY_CLEARANCE_ANY | SHRAY_CLEARANCE_SKIP_SHARED)
{
    if (!op)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "clearance params are NULL");
    if (op->struct_size != sizeof(shray_clearance_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_clearance_params.struct_size is %u, this library expects %zu", op->struct_size,
                    sizeof(shray_clearance_params));
    if (op->max_pairs < 0 || op->max_pairs > SHRAY_CLEARANCE_MAX || (op->flags & ~known))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "clearance params out of range (max_pairs %d of 0 .. %d, flags 0x%x)", op->max_pairs,
                    (int)SHRAY_CLEARANCE_MAX, op->flags);
    return SHRAY_OK;
}

inline int check_any(const shray_clearance_params *op, const void *counts)
{
    if ((op->flags & SHRAY_CLEARANCE_ANY) && (op->max_pairs != 0 || !counts))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "SHRAY_CLEARANCE_ANY needs max_pairs 0 (it is %d) and counts", op->max_pairs);
    return SHRAY_OK;
}

}   // namespace
