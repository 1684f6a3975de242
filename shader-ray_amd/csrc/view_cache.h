// view_cache.h -- a scene's view cache (view_cache.hip): its key and entries, and the steps of a launch that use it
// (render_api.hip: launch_stack_views).  Host-only, internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"
#include "scene_buffers.h"

struct shray_scene;

namespace shray {

// View cache: what a fixed camera's frames have in common, kept per scene.  In the viewer a drag turns the object or the
// light and only the zoom rewrites the camera, so frame after frame the kernels made the same width * height primary
// directions, and for every pixel whose primary ray leaves the scene the same environment lookup and tone map.  An entry
// holds both for one ViewKey, per pixel at its row-major output index (kernel_view_cache.hip writes them, with the frame
// kernels' own functions: the same bits); the timed one-sample instances read them through FrameView::view_rays / view_sky
// (uniform_driver.h).  Only whole plain one-sample frames of kernel 0 are eligible (spp == 1, which == 0, no tile set, no
// tallies): every other launch is what it was.
// Policy: an entry is built -- one prepass kernel on the launch's own stream, in front of the frame kernel -- when a frame
// carries a key that an earlier launch carried lately, and not before: the scene remembers the last kViewEntries distinct
// keys (`view_recent`), so a camera that stands still is cached from its second launch on, one that alternates between
// two positions from its third and fourth, and one that moves every launch (or cycles through more positions than there
// are entries) pays a few key comparisons on the host and nothing else.  kViewEntries entries, least recently used out; an entry larger than
// SHRAY_VIEW_CACHE_MAX_MB (default 256; 28 bytes per pixel, 58 MB at 1920x1080) is not built, and the entries together
// stay below it.  The launch that builds an entry, and later launches on its stream, use it in stream order; launches on
// other streams use it once its `ready` event has been seen complete (polled: no stream waits for another) and until then
// carry null pointers -- the frame is the same either way.
// An evicted or invalidated entry's buffers are set aside in the same kind of list as a dispatch order's
// (shray_scene::view_retired, scene_buffers.h: RetiredPairs): launches that were enqueued before may still read them, so they
// are freed or handed out again only once those launches are over (launch_is_over); nothing synchronises with the device.
struct ViewKey {                        // compared as bytes (no padding: 160 bytes)
    int32_t width, height, spp, tonemap;
    float camera_matrix[16], camera_normal_matrix[16];
    float image_plane_width, aspect;
    uint64_t env_generation;
};
struct ViewEntry {
    ViewKey key{};
    DeviceBuffer rays, sky;             // 3 and 4 floats per pixel
    size_t pixels = 0;                  // 0: the slot holds no entry
    hipEvent_t ready = nullptr;         // recorded behind the prepass
    bool ready_known = false;           // `ready` has been seen complete
    hipStream_t built_on = nullptr;     // launches enqueued on it afterwards are ordered behind the prepass
    unsigned long long last_use = 0;    // launch number
};
constexpr int kViewEntries = 2;

// the entries a launch builds: frame[k] of the launch fills entry[k]
struct ViewBuilds {
    int count = 0;
    int frame[kViewEntries];
    ViewEntry *entry[kViewEntries];
};

// A launch's step 3: gives the eligible frames of launch `seq` their cached tables (staged[k].view_rays / view_sky) and decides
// which entries the launch builds (*builds), which view_cache_fill then fills.  A launch that is not the cache's kind (one
// frame, another kernel, tallies, the cache switched off) gets nothing and builds nothing.
void view_cache_attach(shray_scene *scene, const FrameView *views, int count, FrameView *staged, unsigned long long seq, hipStream_t stream,
                       bool tally, ViewBuilds *builds);

// A launch's step 5: the prepass of every entry in `builds`, behind the upload of the frames' views to d_views (`uploaded`: it
// was enqueued) and in front of the frame kernel.  An entry that is not filled leaves the cache again: no later launch may
// find it.  A failed upload is the caller's to report.
int view_cache_fill(shray_scene *scene, const ViewBuilds &builds, const FrameView *views, const FrameView *d_views, bool uploaded,
                    hipStream_t stream);

// every entry leaves and the recent keys are forgotten (a new environment; shray_scene_set_view_cache(scene, 0))
void view_cache_invalidate(shray_scene *scene);

}   // namespace shray
