// multihit.hip -- include/shader_ray_multihit.h: every crossing of a caller-supplied ray with a resident scene, counted, the
// first K kept in order.
//
// One lane per ray in one-wave workgroups.  The walk reads the 32-byte records of octant copy 7 of the packed tree
// (packed_layout.h: entry planes = boxmin, exit planes = boxmax; the slab test selects per axis by d >= 0, as the shader's
// range_intersect_box does) and the corners from the scene's positions.  Its stack lies in LDS, level-major, one entry per
// edge of the tree's height, as point/point_walk.h's (point/packed_walk.h has what the two walks share).  The crossing set does not depend on the visit order (the header), so
// the walk visits the child with the smaller r0 first, and the form that is not asked for counts skips a node whose r0 is
// above the K-th smallest t held: nothing in it can enter the first K.
//
// multihit/all_hits_walk.h has the walk itself (the instanced form, instance_multihit/, runs it too) and the K best.
// This library is built apart from libshray_hip.so, so the renderer's code objects do not change.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "all_hits_walk.h"
#include "client_internal.h"
#include "first_k_query.h"
#include "multihit_host.h"
#include "packed_walk.h"
#include "shader_ray_multihit.h"
#include "trace_common.h"

using namespace shray;

namespace {

struct MultiWork {
    const float4 *rays;   // 2 float4 per ray
    float4 *hits;         // k per ray: (t, u, v, triangle bits); not touched when k == 0
    int32_t *counts;      // one per ray, or nullptr
    uint64_t count;
    uint64_t first;       // this launch's first ray
    int32_t k;            // records per ray
    int32_t max_leaf_tests;
    DeviceCounters *counters;
};

// One lane per ray.  SLOTS: the register slots of the K best (k <= SLOTS), kSlotsInMemory: they live in the ray's output
// slots (any k, also 0).  PRUNE: skip nodes that cannot reach the first k (no count is written).  COUNT: the work counters.
template <int SLOTS, bool PRUNE, bool COUNT>
__global__ void __launch_bounds__(kBlock) all_hits_kernel(SceneView sc, MultiWork w)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    uint32_t *column = lds_stack + threadIdx.x;   // node names, level-major
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (live) {
        ra = w.rays[2 * index];
        rb = w.rays[2 * index + 1];
    }
    const V3 P = mk(ra.x, ra.y, ra.z), D = mk(rb.x, rb.y, rb.z);
    const float tmax = ra.w;
    const bool traced = live && tmax > 0.0f;   // (false for NaN)
    KBest<SLOTS, false> best;
    best.init(tmax, w.k, w.hits + index * (uint64_t)w.k, nullptr, live);   // (this ray's own slots)
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    if (traced)
        all_hits_walk<SLOTS, PRUNE, false>(sc, P, D, tmax, w.max_leaf_tests, 0, column, best, rc);
    if (live) {
        best.store(nullptr);
        if (w.counts)
            w.counts[index] = best.n;
    }
    if (COUNT)
        add_counters(rc, w.counters);   // (every lane of the wave is here)
}

constexpr Nouns kNouns = {"ray", "rays", "scene", "hits", "max_hits", "all-hits ray query"};

int trace_device(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(kNouns, scene, mp, d_rays, count, d_hits, d_counts);
    if (rc)
        return rc;
    const int k = mp->max_hits;
    if (!aligned(d_rays, 16) || (k > 0 && !aligned(d_hits, 16)) || (d_counts && !aligned(d_counts, 4)))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned, the counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    if ((rc = enter_walkable_scene(scene, &q, &height)))
        return rc;
    MultiWork w{(const float4 *)d_rays, k > 0 ? (float4 *)d_hits : nullptr, d_counts, (uint64_t)count, 0, k, mp->max_leaf_tests, d_counters};
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint32_t);
    return first_k_launches(kNouns, w, count, [&](dim3 grid) {
        with_slots(k, [&](auto slots) {
            with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                hipLaunchKernelGGL((all_hits_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value>), grid, dim3(kBlock),
                                   lds, stream, q.view, w);
            });
        });
    });
}

// the blocking forms: the rays to the device, the query on the null stream, the records, counts (and tallies) back
int trace_host(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count, shray_hit *hits,
               int32_t *counts, shray_counters *out)
{
    if (const int rc = check_query(kNouns, scene, mp, rays, count, hits, counts))
        return rc;
    return first_k_blocking(
        {rays, sizeof(shray_ray), hits, sizeof(shray_hit), nullptr, counts}, count, mp->max_hits, out,
        [&] {
            ShrayQueryScene q;
            int height = 0;
            return enter_walkable_scene(scene, &q, &height);
        },
        [&](void *d_rays, void *d_hits, int32_t *, int32_t *d_counts, DeviceCounters *shards) {
            return trace_device(scene, mp, (const shray_ray *)d_rays, count, (shray_hit *)d_hits, d_counts, nullptr, shards);
        });
}

}   // namespace

extern "C" {

void shray_multihit_params_init(shray_multihit_params *mp)
{
    if (!mp)
        return;
    mp->struct_size = sizeof(shray_multihit_params);
    mp->max_hits = 8;
    mp->max_leaf_tests = 10;   // fs:405
    mp->reserved = 0;
}

int shray_trace_all_hits_device(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count,
                                shray_hit *d_hits, int32_t *d_counts, void *hip_stream)
{
    return trace_device(scene, mp, d_rays, count, d_hits, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_all_hits(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count, shray_hit *hits,
                         int32_t *counts)
{
    return trace_host(scene, mp, rays, count, hits, counts, nullptr);
}

int shray_trace_all_hits_counters(shray_scene *scene, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                                  shray_hit *hits, int32_t *counts, shray_counters *out)
{
    const int rc = check_counters(out);
    return rc ? rc : trace_host(scene, mp, rays, count, hits, counts, out);
}

}   // extern "C"
