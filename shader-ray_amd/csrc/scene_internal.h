// scene_internal.h -- struct shray_scene, the state behind the handle of include/shader_ray_hip.h, as the units of
// libshray_hip.so share it: scene_create.hip fills it, render_api.hip launches from it (with dispatch_order.hip and
// view_cache.hip), capi.hip uploads its environment, hands its parts to the client libraries and destroys it.
// DeviceBuffer and the rule for reusing what launches read are scene_buffers.h's.  Host-only, internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

#include "device_types.h"
#include "dispatch_order.h"
#include "scene_buffers.h"
#include "shader_ray_hip.h"
#include "view_cache.h"

struct shray_scene {
    using DeviceBuffer = shray::DeviceBuffer;
    using FrameView = shray::FrameView;

    int device = 0;
    int kernel_id = 0;          // 0 = stack kernel, 1 = literal threaded kernel, 2 = pool kernel (waves merge)
    bool packed_ok = false;     // link tables verified against the packed tree
    int stack_levels = 1;

    DeviceBuffer positions, normals16, normals32, boxmin, boxmax, hitmiss, objects;
    DeviceBuffer packed_nodes, packed_tris, pair_nodes;
    uint32_t max_leaf_count = 0;     // the largest leaf: the pair records keep min(count, 127) (packed_layout.h)
    DeviceBuffer flat_of_packed;     // int32 per packed node: its number in the flattener's arrays (boxmin, boxmax, objects);
                                     // recorded when packed_ok, for the refit (scene_access_internal.h)
    std::shared_ptr<void> refit_state;   // what libshray_refit.so keeps for this scene (its level order, scratch): freed with it
    std::shared_ptr<void> point_state;   // what libshray_point.so keeps for this scene (the tree's height): freed with it
    std::shared_ptr<void> sdf_state;     // what libshray_sdf.so keeps for this scene (the sign data, its generation): freed with it
    std::shared_ptr<void> winding_state; // what libshray_winding.so keeps for this scene (the node records, their generation): freed with it
    uint64_t geometry_generation = 0;    // bumped by every refit that writes new positions (scene_access_internal.h)
    DeviceBuffer env;
    DeviceBuffer counters;

    // the ring of slots the per-frame FrameViews travel through (scene_buffers.h: kBatchSlots)
    FrameView *batch_staging = nullptr;   // pinned host, kBatchSlots * SHRAY_MAX_BATCH
    DeviceBuffer batch_views;             // device, same shape
    hipEvent_t batch_done[shray::kBatchSlots] = {};
    bool batch_pending[shray::kBatchSlots] = {};

    // the dispatch order (dispatch_order.h):
    // a few shapes side by side (a caller that alternates between two frame sizes or tile sets keeps both orders; a new
    // shape beyond that evicts the least recently used one: its buffers are set aside until the launches that may read
    // them are over (`retired`), nothing synchronises)
    static constexpr int kDispatchShapes = 4;
    shray::DispatchOrder dispatch[kDispatchShapes];
    int dispatch_last = -1;                 // the shape of the most recent ordered launch (shray_scene_dispatch_order)
    unsigned long long dispatch_clock = 0;
    unsigned long long launch_seq = 0;      // launches through launch_stack_views, 1-based; launch q uses batch slot (q - 1) % kBatchSlots
    shray::RetiredPairs retired;            // evicted shapes' (cost, ring), sized in patches
    // a caller that rotates more shapes than there are slots would evict on every launch: shapes that come back after
    // their eviction are counted (the last kEvictedKeys evicted keys are remembered), and after kThrashLimit of them without
    // a launch that found its shape in place the scene's launches keep row-major order for the next kThrashPause launches
    static constexpr int kEvictedKeys = 8, kThrashLimit = 8;
    static constexpr unsigned long long kThrashPause = 256;
    long long evicted_keys[kEvictedKeys][8] = {};
    int evicted_next = 0;
    int dispatch_returns = 0;               // evicted shapes that came back, since the last launch that found its shape in place
    unsigned long long dispatch_paused_until = 0;   // launch number; ordering is off below it

    // kernel id 4 (wavefront form): path queues, counts and per-sample radiances, grown on demand; one launch of a
    // scene at a time uses them (launches on different streams are ordered by wf_done)
    DeviceBuffer wf_queue0, wf_queue1, wf_counts, wf_radiance;
    size_t wf_paths = 0;
    hipEvent_t wf_done = nullptr;
    bool wf_pending = false;

    // shray_render / shray_render_host_async: the device frame is kept between calls (grown on demand),
    // and the blocking form's readback runs on the scene's own stream
    DeviceBuffer frame;
    size_t frame_bytes = 0;
    hipStream_t readback_stream = nullptr;

    // the view cache (view_cache.h)
    shray::ViewEntry view_entries[shray::kViewEntries];
    shray::RetiredPairs view_retired;       // entries' (rays, sky) that left, sized in pixels
    shray::ViewKey view_recent[shray::kViewEntries] = {};  // the last kViewEntries distinct keys that launches carried, most recent first
    int view_recent_count = 0;
    bool view_cache_on = true;              // shray_scene_set_view_cache
    uint64_t env_generation = 0;            // bumped by every environment upload
    uint64_t view_entries_built = 0, view_launches_cached = 0;   // shray_scene_view_cache_stats

    shray::SceneView view{};

    ~shray_scene()
    {
        for (shray::ViewEntry &e : view_entries)
            if (e.ready)
                (void)hipEventDestroy(e.ready);
        if (readback_stream)
            (void)hipStreamDestroy(readback_stream);
        if (wf_done)
            (void)hipEventDestroy(wf_done);
        for (shray::DispatchOrder &d : dispatch)
            for (hipEvent_t e : d.ready)
                if (e)
                    (void)hipEventDestroy(e);
        for (int k = 0; k < shray::kBatchSlots; k++)
            if (batch_done[k])
                (void)hipEventDestroy(batch_done[k]);
        if (batch_staging)
            (void)hipHostFree(batch_staging);
    }
};
