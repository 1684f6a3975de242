// instance.hip -- include/shader_ray_instance.h's queries: world-space rays through a set of placed scenes.
//
// The kernel walks the set's top level wave-uniformly (top_level.h's walk_top_level), and at each leaf the lanes whose rays
// enter the leaf's box move their rays into the instance's object space and run the ray query's walk
// (query/query_common.h: the packed stack traversal in its convergent form), starting from the ray's best hit so far.
// DESIGN.md section 10 argues the box margin and the uniformity of the views.  The set and its build are instance_set.hip's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "error_internal.h"
#include "kernel_stack_common.h"
#include "query_common.h"
#include "set_internal.h"

using namespace shray;
using namespace shray_set;

namespace {

// One-wave workgroups, as query_stack_kernel.  COUNT: the counting instance (closest-hit walks, the compiler's node stage).
template <bool COUNT, bool ANY_HIT>
__global__ void __launch_bounds__(kBatchBlock, COUNT ? SHRAY_MIN_WAVES_VIEW : SHRAY_MIN_WAVES_DEALT)
    instance_kernel(QueryWork w, const TopNode *__restrict__ nodes, const float4 *__restrict__ records,
                    const SceneView *__restrict__ views, int32_t *__restrict__ instances, FrameView fr, int stack_levels,
                    uint32_t top_offset)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    using Traversal = StackTraversal<kBatchBlock, true, false, false, false>;
    Traversal trav = make_traversal<true, kBatchBlock, false, false, false>(lds_stack, stack_levels);
    uint32_t *top = lds_stack + top_offset;   // the wave's top-level stack, after the traversal's LDS
    V3 P = mk(0, 0, 0), D = mk(0, 0, 1);
    float tmax = 0.0f;
    uint64_t index = 0;
    const bool live = query_ray<8>(fr, w, w.first_block + blockIdx.x, P, D, tmax, index);
    const bool traced = live && tmax > 0.0f;   // (false for NaN)
    Hit best{traced ? start_bound(tmax) : kFar, -1.0f, 0.0f, 0.0f};
    int best_instance = -1;
    bool active = traced;   // the ray walks on
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    const float pmax = fmaxf(fabsf(P.x), fmaxf(fabsf(P.y), fabsf(P.z)));
    const unsigned long long first = wave_ballot(active);
    if (first) {
        const uint32_t signs = first_lane_signs(D, first);
        walk_top_level(
            nodes, top,
            [&](uint32_t node, const float4 &a, const float4 &b) { return active && (node == 0u || enters_box(a, b, P, D, a.w * pmax, best.t)); },
            [&](uint32_t link, uint32_t, unsigned long long) -> bool { return (signs >> (link >> 29)) & 1u; },
            [&](int inst, bool enters) {
                const SceneView &sc = leaf_view(records, views, inst);
                V3 Po, Do;
                object_ray(records + 4u * (uint32_t)inst, P, D, Po, Do);
                // a lower instance wins a tie at the best t: its walk may accept t == best.t
                float start = best.t;
                if (best_instance > inst)
                    start = fminf(nextafterf(best.t, INFINITY), kRangeMax);
                Hit h{start, -1.0f, 0.0f, 0.0f};
                trav.template closest<COUNT, ANY_HIT && !COUNT>(sc, fr, enters, Po, Do, h, rc, start);
                if (enters) {
                    if (h.t == -1.0f) {          // the iteration cap: the ray ends
                        best = h;
                        best_instance = -1;
                        active = false;
                    } else if (h.which >= 0.0f && h.t < start) {
                        best = h;
                        best_instance = inst;
                        if (ANY_HIT && !COUNT)
                            active = false;
                    }
                }
            });
    }
    if (live) {
        w.hits[index] = hit_record(best, traced, tmax);
        if (instances)
            instances[index] = best_instance;
    }
    if (COUNT) {
        if (traced && best.t == -1.0f)
            rc.bad_hits++;
        add_counters(rc, w.counters);
    }
}

int trace_device(shray_instance_set *set, const shray_query_params *qp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 int32_t *d_instances, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!set || !d_rays || !d_hits)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, rays or hits is NULL");
    if (!aligned(d_rays, 16) || !aligned(d_hits, 16) || !aligned(d_instances, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned, the instance buffer 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    rc = use_device(set->host.device);
    if (rc)
        return rc;
    const FrameView fr = query_frame(qp);
    const int levels = set->host.stack_levels;
    const size_t walk_lds = stack_lds_bytes(levels, kBatchBlock), lds = walk_lds + kTopStack * sizeof(uint32_t);
    const uint32_t top_offset = (uint32_t)(walk_lds / sizeof(uint32_t));
    const uint64_t blocks = ((uint64_t)count + kBatchBlock - 1) / kBatchBlock, per_launch = kRaysPerLaunch / kBatchBlock;
    QueryWork w{(const float4 *)d_rays, (float4 *)d_hits, (uint64_t)count, 0, d_counters};
    const SetDevice &d = set->dev;
    return for_each_launch(blocks, per_launch, [&](uint64_t first, dim3 grid) {
        w.first_block = first;
        if (d_counters)
            hipLaunchKernelGGL((instance_kernel<true, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else if (qp->any_hit)
            hipLaunchKernelGGL((instance_kernel<false, true>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else
            hipLaunchKernelGGL((instance_kernel<false, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        return launched("instance query");
    });
}

// the blocking forms: the rays to the device, the query on the null stream, the results (and tallies) back
int trace_host(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count, shray_hit *hits,
               int32_t *instances, shray_counters *out)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!set || !rays)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or rays is NULL");
    if (out) {
        memset(out, 0, sizeof(*out));
        out->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    rc = use_device(set->host.device);
    if (rc)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{rays, n * sizeof(shray_ray)}}, {{hits, n * sizeof(shray_hit)}, {instances, instances ? n * sizeof(int32_t) : 0}}, out,
                        [&](DeviceBuffer *d_rays, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return trace_device(set, qp, d_rays->as<const shray_ray>(), count, d_out[0].as<shray_hit>(),
                                                d_out[1].as<int32_t>(), nullptr, shards);
                        });
}

}   // namespace

extern "C" {

int shray_trace_instances_device(shray_instance_set *set, const shray_query_params *qp, const shray_ray *d_rays, int64_t count,
                                 shray_hit *d_hits, int32_t *d_instances, void *hip_stream)
{
    return trace_device(set, qp, d_rays, count, d_hits, d_instances, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_instances(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                          shray_hit *hits, int32_t *instances)
{
    if (!hits && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "hits is NULL");
    return trace_host(set, qp, rays, count, hits, instances, nullptr);
}

int shray_trace_instances_counters(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                                   shray_hit *hits, int32_t *instances, shray_counters *out)
{
    if (!out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return trace_host(set, qp, rays, count, hits, instances, out);
}

}   // extern "C"
