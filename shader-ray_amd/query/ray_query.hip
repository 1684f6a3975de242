// ray_query.hip -- include/shader_ray_query.h: caller-supplied object-space rays through the scene's BVH, one hit record each.
//
// The walk is the renderer's own, from the product's headers (csrc/): the packed stack traversal in its convergent form
// (StackTraversal::closest: the dealt leaf stage and the hand-scheduled node and leaf stages of the timed instances), or the
// literal threaded traversal (kernel id 1, or a scene without a packed tree).  The one difference from the shader's traversal
// is where the running closest hit starts: at the ray's tmax (clamped to the range's end, 1e8 -- see the header) instead of
// infinitely_far.  This library is built apart from libshray_hip.so, so the renderer's code objects do not change.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "client_internal.h"
#include "error_internal.h"
#include "kernel_stack_common.h"
#include "query_common.h"
#include "scene_access_internal.h"
#include "shader_ray_query.h"
#include "threaded_traversal.h"

using namespace shray;

namespace {

constexpr int kThreadedBlock = 256;

// kernel id 0: one-wave workgroups, the convergent packed stack traversal (every lane of the wave enters closest() together).
// COUNT: the counting instance (the compiler's node stage, the cap in front of every visit, every ray walked to its end).
template <bool COUNT, bool ANY_HIT>
__global__ void __launch_bounds__(kBatchBlock, COUNT ? SHRAY_MIN_WAVES_VIEW : SHRAY_MIN_WAVES_DEALT)
    query_stack_kernel(SceneView sc, FrameView fr, QueryWork w, int stack_levels)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    using Traversal = StackTraversal<kBatchBlock, true, false, false, false>;
    Traversal trav = make_traversal<true, kBatchBlock, false, false, false>(lds_stack, stack_levels);
    V3 P = mk(0, 0, 0), D = mk(0, 0, 1);
    float tmax = 0.0f;
    uint64_t index = 0;
    const bool live = query_ray<8>(fr, w, w.first_block + blockIdx.x, P, D, tmax, index);
    const bool traced = live && tmax > 0.0f;   // (false for NaN)
    const float bound = traced ? start_bound(tmax) : kFar;
    Hit hit{bound, -1.0f, 0.0f, 0.0f};
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    trav.template closest<COUNT, ANY_HIT && !COUNT>(sc, fr, traced, P, D, hit, rc, bound);
    if (live)
        w.hits[index] = hit_record(hit, traced, tmax);
    if (COUNT) {
        if (traced && hit.t == -1.0f)
            rc.bad_hits++;
        add_counters(rc, w.counters);
    }
}

// kernel id 1: the literal threaded traversal, one ray per thread (any-hit rays are walked to their end: the closest hit is
// an any-hit answer)
template <bool COUNT>
__global__ void __launch_bounds__(kThreadedBlock) query_threaded_kernel(SceneView sc, FrameView fr, QueryWork w)
{
    V3 P = mk(0, 0, 0), D = mk(0, 0, 1);
    float tmax = 0.0f;
    uint64_t index = 0;
    const bool live = query_ray<16>(fr, w, w.first_block + blockIdx.x, P, D, tmax, index);
    const bool traced = live && tmax > 0.0f;
    Hit hit{traced ? start_bound(tmax) : kFar, -1.0f, 0.0f, 0.0f};
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    ThreadedTraversal trav;
    if (traced)
        trav.closest<COUNT>(sc, fr, P, D, hit, rc);
    if (live)
        w.hits[index] = hit_record(hit, traced, tmax);
    if (COUNT) {
        if (traced && hit.t == -1.0f)
            rc.bad_hits++;
        add_counters(rc, w.counters);   // (every lane of the wave is here)
    }
}

// `blocks` workgroups of work `w` (first_block = 0), in launches of at most kRaysPerLaunch threads
int launch_query(const ShrayQueryScene &q, const FrameView &fr, QueryWork w, uint64_t blocks, bool any_hit, hipStream_t stream)
{
    const bool stack = q.packed_ok && q.kernel_id != 1;
    const int block = stack ? kBatchBlock : kThreadedBlock;
    const uint64_t per_launch = kRaysPerLaunch / (uint64_t)block;
    const size_t lds = stack ? stack_lds_bytes(q.stack_levels, kBatchBlock) : 0;
    const bool count = w.counters != nullptr;
    return for_each_launch(blocks, per_launch, [&](uint64_t first, dim3 grid) {
        w.first_block = first;
        if (stack && count)
            hipLaunchKernelGGL((query_stack_kernel<true, false>), grid, dim3(block), lds, stream, q.view, fr, w, q.stack_levels);
        else if (stack && any_hit)
            hipLaunchKernelGGL((query_stack_kernel<false, true>), grid, dim3(block), lds, stream, q.view, fr, w, q.stack_levels);
        else if (stack)
            hipLaunchKernelGGL((query_stack_kernel<false, false>), grid, dim3(block), lds, stream, q.view, fr, w, q.stack_levels);
        else if (count)
            hipLaunchKernelGGL((query_threaded_kernel<true>), grid, dim3(block), 0, stream, q.view, fr, w);
        else
            hipLaunchKernelGGL((query_threaded_kernel<false>), grid, dim3(block), 0, stream, q.view, fr, w);
        return launched("ray query");
    });
}

int trace_device(shray_scene *scene, const shray_query_params *qp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!scene || !d_rays || !d_hits)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, rays or hits is NULL");
    if (!aligned(d_rays, 16) || !aligned(d_hits, 16))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    rc = enter_scene(scene, &q);
    if (rc)
        return rc;
    const bool stack = q.packed_ok && q.kernel_id != 1;
    const uint64_t block = stack ? kBatchBlock : kThreadedBlock;
    QueryWork w{(const float4 *)d_rays, (float4 *)d_hits, (uint64_t)count, 0, d_counters};
    return launch_query(q, query_frame(qp), w, ((uint64_t)count + block - 1) / block, qp->any_hit != 0, stream);
}

// the blocking forms: the rays to the device, the query on the null stream, the hits (and tallies) back
int trace_host(shray_scene *scene, const shray_query_params *qp, const shray_ray *rays, int64_t count, shray_hit *hits,
               shray_counters *out)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!scene || !rays || (!hits && !out))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, rays or hits is NULL");
    if (out) {
        memset(out, 0, sizeof(*out));
        out->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    rc = enter_scene(scene, &q);
    if (rc)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{rays, n * sizeof(shray_ray)}}, {{hits, n * sizeof(shray_hit)}}, out,
                        [&](DeviceBuffer *d_rays, DeviceBuffer *d_hits, DeviceCounters *shards) {
                            return trace_device(scene, qp, d_rays->as<const shray_ray>(), count, d_hits->as<shray_hit>(), nullptr, shards);
                        });
}

}   // namespace

extern "C" {

void shray_query_params_init(shray_query_params *qp)
{
    if (!qp)
        return;
    qp->struct_size = sizeof(shray_query_params);
    qp->max_bvh_iterations = 400;   // fs:426
    qp->max_leaf_tests = 10;        // fs:405
    qp->any_hit = 0;
}

int shray_trace_rays_device(shray_scene *scene, const shray_query_params *qp, const shray_ray *d_rays, int64_t count,
                            shray_hit *d_hits, void *hip_stream)
{
    return trace_device(scene, qp, d_rays, count, d_hits, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_rays(shray_scene *scene, const shray_query_params *qp, const shray_ray *rays, int64_t count, shray_hit *hits)
{
    if (!hits && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "hits is NULL");
    return trace_host(scene, qp, rays, count, hits, nullptr);
}

int shray_trace_rays_counters(shray_scene *scene, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                              shray_hit *hits, shray_counters *out)
{
    if (!out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return trace_host(scene, qp, rays, count, hits, out);
}

int shray_primary_hits_device(shray_scene *scene, const shray_frame_params *params, int width, int height, shray_hit *d_hits,
                              void *hip_stream)
{
    if (!scene || !params || !d_hits)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, params or hits is NULL");
    if (!aligned(d_hits, 16))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the hit buffer must be 16-byte aligned");
    FrameView fr;
    int rc = shrayi_frame_view(params, width, height, &fr);
    if (rc)
        return rc;
    ShrayQueryScene q;
    rc = enter_scene(scene, &q);
    if (rc)
        return rc;
    const uint64_t tile = (q.packed_ok && q.kernel_id != 1) ? 8u : 16u;
    const uint64_t blocks = (((uint64_t)width + tile - 1) / tile) * (((uint64_t)height + tile - 1) / tile);
    QueryWork w{nullptr, (float4 *)d_hits, (uint64_t)width * (uint64_t)height, 0, nullptr};
    return launch_query(q, fr, w, blocks, false, (hipStream_t)hip_stream);
}

}   // extern "C"
