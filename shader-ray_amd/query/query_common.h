// query_common.h -- what the ray query (ray_query.hip) and the instanced query (instance/instance.hip) share: a launch's work,
// how a lane reads its ray, the hit record a walk's result becomes, the walk's starting bound, the parameter check and the
// query's FrameView.  Internal to those libraries; include/shader_ray_query.h states the semantics.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "error_internal.h"
#include "kernel_stack_common.h"
#include "shader_ray_query.h"

namespace {

using namespace shray;

// rays per launch: a larger count is split (the grid's threads must stay below 2^32; and a launch of this size fills the
// machine many times over, so the split costs nothing measurable)
constexpr uint64_t kRaysPerLaunch = 1ull << 24;

// What a kernel works on: rays from memory, or the primary rays of a frame in 8 x 8 (stack) / 16 x 16 (threaded) pixel tiles.
struct QueryWork {
    const float4 *rays;   // 2 float4 per ray; nullptr: primary rays of `fr`
    float4 *hits;         // (t, u, v, triangle bits)
    uint64_t count;       // rays, or pixels
    uint64_t first_block; // of this launch
    DeviceCounters *counters;
};

// The ray of work item i, or the pixel ray of the lane in tile `tile`.  Returns false for a lane without a work item.
template <int TILE>
__device__ __forceinline__ bool query_ray(const FrameView &fr, const QueryWork &w, uint64_t block, V3 &P, V3 &D, float &tmax,
                                          uint64_t &index)
{
    if (w.rays) {
        index = block * (uint64_t)(TILE * TILE) + threadIdx.x;
        if (index >= w.count)
            return false;
        const float4 a = w.rays[2 * index], b = w.rays[2 * index + 1];
        P = mk(a.x, a.y, a.z);
        tmax = a.w;
        D = mk(b.x, b.y, b.z);
        return true;
    }
    // trace_pixels (trace_common.h) at one sample: the pixel-centre ray, then the object transform of trace_ray
    const unsigned int tiles_x = ((unsigned int)fr.width + TILE - 1u) / TILE;
    const int px = (int)((block % tiles_x) * TILE + threadIdx.x % TILE);
    const int py = (int)((block / tiles_x) * TILE + threadIdx.x / TILE);
    if (px >= fr.width || py >= fr.height)
        return false;
    index = (uint64_t)py * (uint64_t)fr.width + (uint64_t)px;
    const float u = ((float)px + 0.5f) / (float)fr.width;
    const float v = ((float)py + 0.5f) / (float)fr.height;
    const V3 eye = unit(mk(fr.image_plane_width * (u - 0.5f), fr.image_plane_width * (v - 0.5f) * fr.aspect, -1.0f));
    const V3 Pw = xform(fr.camera_matrix, mk(0, 0, 0), 1.0f);
    const V3 Dw = unit(xform(fr.camera_normal_matrix, eye, 0.0f));
    P = xform(fr.object_matrix, Pw, 1.0f);
    D = xform(fr.object_normal_matrix, Dw, 0.0f);
    tmax = kFar;
    return true;
}

// The walk's result as a hit record (header: semantics).  traced = the ray was walked (tmax > 0).
__device__ __forceinline__ float4 hit_record(const Hit &hit, bool traced, float tmax)
{
    int triangle;
    float t = hit.t;
    if (traced && hit.t == -1.0f) {
        triangle = SHRAY_HIT_CAP;
    } else if (traced && hit.which >= 0.0f && hit.t < tmax) {
        triangle = (int)hit.which;
    } else {
        triangle = SHRAY_HIT_MISS;
        if (!(hit.which >= 0.0f))
            t = tmax;   // nothing accepted: the bound the walk started from (before its clamp to the range's end)
    }
    return make_float4(t, hit.bu, hit.bv, __int_as_float(triangle));
}

// the walk starts from min(tmax, 1e8) (the header explains why that is the same walk)
__device__ __forceinline__ float start_bound(float tmax) { return tmax < kRangeMax ? tmax : kRangeMax; }

int check_params(const shray_query_params *qp)
{
    if (!qp)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "query params are NULL");
    if (qp->struct_size != sizeof(shray_query_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_query_params.struct_size is %u, this library expects %zu", qp->struct_size,
                    sizeof(shray_query_params));
    if (qp->max_bvh_iterations < 0 || qp->max_bvh_iterations > (1 << 24) || qp->max_leaf_tests < 0 || qp->max_leaf_tests > (1 << 24) ||
        (qp->any_hit != 0 && qp->any_hit != 1))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "query params out of range (max_bvh_iterations %d, max_leaf_tests %d, any_hit %d)",
                    qp->max_bvh_iterations, qp->max_leaf_tests, qp->any_hit);
    return SHRAY_OK;
}

// the query's FrameView: only the traversal's two constants are read (0 = no cap: a cap nothing reaches)
FrameView query_frame(const shray_query_params *qp)
{
    FrameView fr;
    memset(&fr, 0, sizeof(fr));
    fr.max_bvh_iterations = qp->max_bvh_iterations > 0 ? qp->max_bvh_iterations : INT_MAX;
    fr.max_leaf_tests = qp->max_leaf_tests;
    return fr;
}

}   // namespace
