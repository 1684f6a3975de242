// view_cache.hip -- a scene's view cache (view_cache.h): the key of a frame, which launches are the cache's kind, where an
// entry's buffers come from and go to, and the entry points that switch the cache and report on it.  Host code only; the
// prepass that fills an entry is kernel_view_cache.hip's (launch_view_cache).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "error_internal.h"
#include "launch.h"
#include "scene_internal.h"
#include "shader_ray_hip.h"
#include "view_cache.h"

using namespace shray;

namespace {

// The view cache (view_cache.h: ViewEntry).  SHRAY_VIEW_CACHE=0 turns it off for a process (read once);
// shray_scene_set_view_cache for a scene.
bool view_cache_enabled()
{
    static const bool on = [] {
        const char *e = getenv("SHRAY_VIEW_CACHE");
        return !(e && e[0] == '0');
    }();
    return on;
}
// bytes the entries of a scene may hold together (read where an entry is about to be built, not per launch)
size_t view_cache_cap_bytes()
{
    const char *e = getenv("SHRAY_VIEW_CACHE_MAX_MB");
    const long long mb = e ? atoll(e) : 256;
    return mb <= 0 ? 0 : (size_t)mb << 20;
}
constexpr size_t kViewBytesPerPixel = 7 * sizeof(float);

bool view_cache_eligible(const FrameView &f) { return f.spp == 1 && f.which == 0 && f.tile_stride == 0; }

void view_key_of(const FrameView &f, uint64_t env_generation, ViewKey *key)
{
    memset(key, 0, sizeof(*key));
    key->width = f.width;
    key->height = f.height;
    key->spp = f.spp;
    key->tonemap = f.tonemap;
    memcpy(key->camera_matrix, f.camera_matrix, sizeof(key->camera_matrix));
    memcpy(key->camera_normal_matrix, f.camera_normal_matrix, sizeof(key->camera_normal_matrix));
    key->image_plane_width = f.image_plane_width;
    key->aspect = f.aspect;
    key->env_generation = env_generation;
}

// the entry leaves; launches enqueued so far may still read its buffers
void view_entry_retire(shray_scene *scene, ViewEntry &e)
{
    if (!e.pixels)
        return;
    scene->view_retired.push(&e.rays.p, &e.sky.p, e.pixels, scene->launch_seq);
    e.pixels = 0;
}

// A new entry for `key` in launch `seq`: the slot of the least recently used entry that this launch does not read, buffers
// from the retired ones where one fits.  nullptr: nothing is built (over the cap, no slot, no memory) and the frame renders
// uncached.
ViewEntry *view_entry_start(shray_scene *scene, const ViewKey &key, unsigned long long seq, hipStream_t stream)
{
    const size_t pixels = (size_t)key.width * (size_t)key.height, cap = view_cache_cap_bytes();
    if (pixels * kViewBytesPerPixel > cap)
        return nullptr;
    ViewEntry *slot = nullptr;
    for (;;) {
        size_t held = 0;
        ViewEntry *lru = nullptr;
        slot = nullptr;
        for (ViewEntry &e : scene->view_entries) {
            held += e.pixels * kViewBytesPerPixel;
            if (!e.pixels)
                slot = slot ? slot : &e;
            else if (e.last_use != seq && (!lru || e.last_use < lru->last_use))
                lru = &e;
        }
        if (slot && held + pixels * kViewBytesPerPixel <= cap)
            break;
        if (!lru)
            return nullptr;
        view_entry_retire(scene, *lru);
    }
    ViewEntry &e = *slot;
    // retired buffers nobody reads any more: one pair that fits serves this entry, the others are freed
    if (!e.rays.p)
        scene->view_retired.take_first(seq, [&](size_t held) { return held >= pixels && held <= pixels + pixels / 4; }, &e.rays.p, &e.sky.p);
    scene->view_retired.free_aged(seq);
    if (!e.rays.p || !e.sky.p) {
        e.rays.release();
        e.sky.release();
        if (e.rays.reserve(pixels * 3 * sizeof(float)) != hipSuccess || e.sky.reserve(pixels * 4 * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            e.rays.release();
            e.sky.release();
            return nullptr;
        }
    }
    if (!e.ready && hipEventCreateWithFlags(&e.ready, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        e.ready = nullptr;
        e.rays.release();
        e.sky.release();
        return nullptr;
    }
    e.key = key;
    e.pixels = pixels;
    e.ready_known = false;
    e.built_on = stream;    // (the prepass follows on it, in this launch: view_cache_fill)
    e.last_use = seq;
    return &e;
}

int view_entry_fill(shray_scene *scene, ViewEntry &e, const FrameView &fr, const FrameView *d_frame, hipStream_t stream)
{
    const hipError_t err = launch_view_cache(scene->view, d_frame, fr, (float *)e.rays.p, (float *)e.sky.p, stream);
    if (err != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "view-cache kernel launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipEventRecord(e.ready, stream));
    scene->view_entries_built++;
    return SHRAY_OK;
}

}   // namespace

namespace shray {

void view_cache_attach(shray_scene *scene, const FrameView *views, int count, FrameView *staged, unsigned long long seq, hipStream_t stream,
                       bool tally, ViewBuilds *builds)
{
    builds->count = 0;
    // whole plain one-sample frames of the stack kernel's timed instances (the tallying twins never get the tables: their
    // tallies stay the work of an uncached frame)
    // Launches of several frames only.  A lone frame is bound by the latency of its longest waves, not by instructions: with the
    // tables its waves begin with a scalar load and a dependent read of memory no earlier wave of the launch has touched, and
    // the frame was 1.4-2 % SLOWER (0.385 against 0.378-0.380 ms, R9.1); a one-frame launch is what it was.
    if (!(count > 1 && scene->kernel_id == 0 && !tally && scene->view_cache_on && view_cache_enabled()))
        return;
    constexpr int kRecent = kViewEntries;
    ViewKey recent[kRecent + 1];      // the keys seen lately, most recent first, as they will be after this launch
    int recent_count = scene->view_recent_count;
    memcpy(recent, scene->view_recent, sizeof(ViewKey) * (size_t)recent_count);
    bool used = false;
    for (int k = 0; k < count; k++) {
        if (!view_cache_eligible(views[k]))
            continue;
        ViewKey key;
        view_key_of(views[k], scene->env_generation, &key);
        {   // move to the front
            int at = 0;
            while (at < recent_count && memcmp(&recent[at], &key, sizeof(key)) != 0)
                at++;
            if (at == recent_count && recent_count <= kRecent)
                recent_count++;
            for (int j = at < recent_count ? at : recent_count - 1; j > 0; j--)
                recent[j] = recent[j - 1];
            recent[0] = key;
            if (recent_count > kRecent)
                recent_count = kRecent;
        }
        ViewEntry *entry = nullptr;
        for (ViewEntry &e : scene->view_entries)
            if (e.pixels && memcmp(&e.key, &key, sizeof(key)) == 0)
                entry = &e;
        bool fresh = false;
        if (!entry) {
            bool seen = false;     // an earlier launch carried this key lately: the camera stands still, or is back
            for (int j = 0; j < scene->view_recent_count; j++)
                seen = seen || memcmp(&scene->view_recent[j], &key, sizeof(key)) == 0;
            if (!seen || builds->count >= kViewEntries)
                continue;
            entry = view_entry_start(scene, key, seq, stream);
            if (!entry)
                continue;
            builds->frame[builds->count] = k;
            builds->entry[builds->count] = entry;
            builds->count++;
            fresh = true;
        }
        if (!fresh && !entry->ready_known && stream != entry->built_on && hipEventQuery(entry->ready) == hipSuccess)
            entry->ready_known = true;
        (void)hipGetLastError();   // (hipErrorNotReady is no error of this launch)
        if (!(fresh || entry->ready_known || stream == entry->built_on))
            continue;              // still being written on another stream: this frame computes as ever
        entry->last_use = seq;
        staged[k].view_rays = SHRAY_VIEW_CACHE_RAYS ? (const float *)entry->rays.p : nullptr;
        staged[k].view_sky = SHRAY_VIEW_CACHE_SKY ? (const float *)entry->sky.p : nullptr;
        used = true;
    }
    memcpy(scene->view_recent, recent, sizeof(ViewKey) * (size_t)recent_count);
    scene->view_recent_count = recent_count;
    if (used)
        scene->view_launches_cached++;
}

int view_cache_fill(shray_scene *scene, const ViewBuilds &builds, const FrameView *views, const FrameView *d_views, bool uploaded,
                    hipStream_t stream)
{
    for (int k = 0; k < builds.count; k++) {
        const int rc = uploaded ? view_entry_fill(scene, *builds.entry[k], views[builds.frame[k]], d_views + builds.frame[k], stream)
                                : SHRAY_ERR_DEVICE;
        if (rc) {
            for (int j = k; j < builds.count; j++)       // never filled: no later launch may find them
                view_entry_retire(scene, *builds.entry[j]);
            return uploaded ? rc : SHRAY_OK;
        }
    }
    return SHRAY_OK;
}

void view_cache_invalidate(shray_scene *scene)
{
    for (ViewEntry &e : scene->view_entries)
        view_entry_retire(scene, e);
    scene->view_recent_count = 0;
}

}   // namespace shray

extern "C" {

int shray_scene_set_view_cache(shray_scene *scene, int on)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    scene->view_cache_on = on != 0;
    if (!on)
        view_cache_invalidate(scene);
    return SHRAY_OK;
}

int shray_scene_view_cache_stats(const shray_scene *scene, uint64_t *entries_built, uint64_t *launches_cached, uint64_t *bytes_held)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (entries_built)
        *entries_built = scene->view_entries_built;
    if (launches_cached)
        *launches_cached = scene->view_launches_cached;
    if (bytes_held) {
        size_t pixels = scene->view_retired.total_size();
        for (const ViewEntry &e : scene->view_entries)
            pixels += e.pixels;
        *bytes_held = (uint64_t)(pixels * kViewBytesPerPixel);
    }
    return SHRAY_OK;
}

}   // extern "C"
