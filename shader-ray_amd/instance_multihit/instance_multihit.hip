// instance_multihit.hip -- include/shader_ray_instance_multihit.h: every crossing of a world-space ray with a set of placed
// scenes, counted, the first K kept in order with their instances.
//
// One lane per ray in one-wave workgroups.  The wave walks the set's top level uniformly (instance/top_level.h's
// walk_top_level, with its widened slab test); at a leaf the lanes whose rays enter its box move their rays into the
// instance's object space and each runs the all-hits walk of that scene (multihit/all_hits_walk.h) into its own K best,
// which carry the instance index as a fifth field.  The cull limit of a lane is its tmax, or, in the form that is not asked
// for counts, the K-th smallest t it holds: the same t_K that prunes the walks inside the scenes.
// This library is built apart from libshray_hip.so, libshray_instance.so and libshray_multihit.so, so their code objects do
// not change.
#include <hip/hip_runtime.h>

#include <cstring>

#include "all_hits_walk.h"
#include "client_internal.h"
#include "enter_set.h"
#include "first_k_query.h"
#include "multihit_host.h"
#include "packed_walk.h"
#include "shader_ray_instance_multihit.h"
#include "top_level.h"
#include "trace_common.h"

using namespace shray;

namespace {

struct SetWork {
    const float4 *rays;    // 2 float4 per ray, world space
    float4 *hits;          // k per ray: (t, u, v, triangle bits); not touched when k == 0
    int32_t *instances;    // k per ray, or nullptr (never nullptr for the form that keeps its K best in memory, k > 0)
    int32_t *counts;       // one per ray, or nullptr
    uint64_t count;
    uint64_t first;        // this launch's first ray
    int32_t k;             // records per ray
    int32_t max_leaf_tests;
    int32_t stack_levels;  // the tallest member scene's height (at least 1): the top-level stack follows the walk's columns
    DeviceCounters *counters;
};

// One lane per ray.  SLOTS, PRUNE, COUNT: as all_hits_kernel's (multihit/multihit.hip).  The pointers are __restrict__ so that
// a leaf's record and its SceneView come in by scalar loads.
template <int SLOTS, bool PRUNE, bool COUNT>
__global__ void __launch_bounds__(kBlock) instance_all_hits_kernel(SetWork w, const TopNode *__restrict__ nodes,
                                                                   const float4 *__restrict__ records,
                                                                   const SceneView *__restrict__ views)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    uint32_t *column = lds_stack + threadIdx.x;                      // node names, level-major
    uint32_t *top = lds_stack + (size_t)kBlock * w.stack_levels;     // the wave's top-level stack
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
    KBest<SLOTS, true> best;
    best.init(tmax, w.k, w.hits + index * (uint64_t)w.k, w.instances + index * (uint64_t)w.k, live);   // (this ray's own slots)
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    const float pmax = fmaxf(fabsf(P.x), fmaxf(fabsf(P.y), fabsf(P.z)));
    const unsigned long long first = __builtin_amdgcn_ballot_w64(traced);
    if (first) {
        const uint32_t signs = first_lane_signs(D, first);
        walk_top_level(
            nodes, top,
            // A lane's limit: nothing beyond tmax is accepted; nothing beyond t_K can enter the first k (a box that begins
            // AT t_K is entered: enters_box keeps tn <= limit, and a lower instance wins a tie there)
            [&](uint32_t node, const float4 &a, const float4 &b) {
                return traced && (node == 0u || enters_box(a, b, P, D, a.w * pmax, PRUNE ? best.tk : tmax));
            },
            [&](uint32_t link, uint32_t, unsigned long long) -> bool { return (signs >> (link >> 29)) & 1u; },
            [&](int inst, bool enters) {
                const SceneView &sc = leaf_view(records, views, inst);
                if (enters) {
                    V3 Po, Do;
                    object_ray(records + 4u * (uint32_t)inst, P, D, Po, Do);
                    all_hits_walk<SLOTS, PRUNE, true>(sc, Po, Do, tmax, w.max_leaf_tests, inst, column, best, rc);
                }
            });
    }
    if (live) {
        best.store(w.instances ? w.instances + index * (uint64_t)w.k : nullptr);
        if (w.counts)
            w.counts[index] = best.n;
    }
    if (COUNT)
        add_counters(rc, w.counters);   // (every lane of the wave is here)
}

constexpr Nouns kNouns = {"ray", "rays", "set", "hits", "max_hits", "instanced all-hits ray query"};

int trace_device(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 int32_t *d_instances, int32_t *d_counts, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_query(kNouns, set, mp, d_rays, count, d_hits, d_counts);
    if (rc)
        return rc;
    const int k = mp->max_hits;
    if (!aligned(d_rays, 16) || (k > 0 && !aligned(d_hits, 16)) || !aligned(d_instances, 4) || !aligned(d_counts, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned, the instances and counts 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    // (rays go into an instance's object space: the forward maps are not asked for)
    return walk_set(set, false, k, count, d_instances, stream, [&](const SetWalk &s) {
        SetWork w{(const float4 *)d_rays, k > 0 ? (float4 *)d_hits : nullptr, k > 0 ? s.instances : nullptr, d_counts, (uint64_t)count, 0, k,
                  mp->max_leaf_tests, s.levels, d_counters};
        const size_t lds = s.lds(sizeof(uint32_t));
        return first_k_launches(kNouns, w, count, [&](dim3 grid) {
            with_slots(k, [&](auto slots) {
                with_form(form_for(d_counters, d_counts, k), [&](auto prune, auto tally) {
                    hipLaunchKernelGGL((instance_all_hits_kernel<decltype(slots)::value, decltype(prune)::value, decltype(tally)::value>), grid,
                                       dim3(kBlock), lds, stream, w, s.nodes, s.records, s.views);
                });
            });
        });
    });
}

// the blocking forms: the rays to the device, the query on the null stream, the records, instances, counts (and tallies) back
int trace_host(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *rays, int64_t count, shray_hit *hits,
               int32_t *instances, int32_t *counts, shray_counters *out)
{
    if (const int rc = check_query(kNouns, set, mp, rays, count, hits, counts))
        return rc;
    return first_k_blocking(
        {rays, sizeof(shray_ray), hits, sizeof(shray_hit), instances, counts}, count, mp->max_hits, out,
        [&] { return enter_set(set); },
        [&](void *d_rays, void *d_hits, int32_t *d_instances, int32_t *d_counts, DeviceCounters *shards) {
            return trace_device(set, mp, (const shray_ray *)d_rays, count, (shray_hit *)d_hits, d_instances, d_counts, nullptr, shards);
        });
}

}   // namespace

extern "C" {

int shray_trace_instances_all_hits_device(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *d_rays,
                                          int64_t count, shray_hit *d_hits, int32_t *d_instances, int32_t *d_counts, void *hip_stream)
{
    return trace_device(set, mp, d_rays, count, d_hits, d_instances, d_counts, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_instances_all_hits(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *rays, int64_t count,
                                   shray_hit *hits, int32_t *instances, int32_t *counts)
{
    return trace_host(set, mp, rays, count, hits, instances, counts, nullptr);
}

int shray_trace_instances_all_hits_counters(shray_instance_set *set, const shray_multihit_params *mp, const shray_ray *rays,
                                            int64_t count, shray_hit *hits, int32_t *instances, int32_t *counts, shray_counters *out)
{
    const int rc = check_counters(out);
    return rc ? rc : trace_host(set, mp, rays, count, hits, instances, counts, out);
}

}   // extern "C"
