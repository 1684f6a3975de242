// render_api.hip -- the render entry points of include/shader_ray_hip.h and the one path every launch of the stack kernel
// takes (launch_stack_views): which instance a launch runs, the ring of slots its FrameViews travel through, and in between
// the steps of dispatch_order.hip and view_cache.hip.  Also the tile-set assembly, the scene's kept frame and readback stream,
// pinned host memory, the read-back of the current dispatch order and the diagnostic timeline.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "counters_internal.h"
#include "device_types.h"
#include "dispatch_order.h"
#include "error_internal.h"
#include "frame_view_host.h"
#include "launch.h"
#include "packed_layout.h"
#include "scene_internal.h"
#include "shader_ray_hip.h"
#include "view_cache.h"

using namespace shray;

namespace {

// Which leaf stage the convergent instances of the stack kernel run.  Dealing a parked ray's triangles to the
// wave's idle lanes shortens divergent waves -- fewer instructions, one memory round trip per leaf instead of up
// to ten -- but the instance holds a second ray's worth of registers: six waves per SIMD instead of eight for the
// spp == 1 gold instance, five instead of six for the diffuse / shadow-ray ones.  Measured on MI355X
// (profiles/history/r02/leaf_stage_ab.txt):
//   * trees larger than an XCD's L2 share (the 1M-triangle scene, 9.4 MB of nodes): rays diverge, the walk is
//     latency-bound, dealing wins by 10-18 %;
//   * one spp == 1 frame per launch (latency): the frame ends with a tail of divergent waves, dealing wins by 11 %;
//   * a cache-resident scene rendered for throughput (several frames per launch, or many samples per pixel):
//     the GPU is full of coherent waves, the extra waves are worth more (3-6 %).
bool leaf_stage_policy(const shray_scene *scene, int frames_in_launch, int spp)
{
    const bool divergent_scene = (size_t)scene->view.group_count * sizeof(PackedNode) > (2u << 20);
    const bool latency_launch = frames_in_launch == 1 && spp == 1;
    return divergent_scene || latency_launch;
}

// Which launches of the stack kernel test both children of a node per turn (variants/pair_traversal.h: inner_stage_pair): those
// of a scene that asked for it, shray_scene_set_kernel(scene, 3).  The pair form issues the same arithmetic and the same
// loads as the one-visit form but about 0.6 of its dependent round trips, for a fatter turn; measured 24-35 % slower on
// every configuration (profiles/EXPERIMENTS.md R3.2), so no launch chooses it by itself.
bool pair_policy(const shray_scene *scene, const FrameView *views, int count)
{
    if (!scene->pair_nodes.p || scene->kernel_id != 3)
        return false;
    // a pair record keeps min(triangle count, 127): exact whenever the leaf cap or the largest leaf stays below that
    for (int k = 0; k < count; k++)
        if (scene->max_leaf_count > 126u && (uint32_t)views[k].max_leaf_tests > 126u)
            return false;
    return true;
}

// kernel id 4 (wavefront form): the scene's queues, counts and event, for a frame of `paths` paths
int ensure_wavefront_queues(shray_scene *scene, size_t paths)
{
    if (scene->wf_paths < paths) {
        HIP_TRY(hipDeviceSynchronize());     // nothing may still be using the old queues
        scene->wf_queue0.release();
        scene->wf_queue1.release();
        scene->wf_radiance.release();
        scene->wf_paths = 0;
        HIP_TRY(hipMalloc(&scene->wf_queue0.p, paths * 64));
        HIP_TRY(hipMalloc(&scene->wf_queue1.p, paths * 64));
        HIP_TRY(hipMalloc(&scene->wf_radiance.p, paths * 16));
        scene->wf_paths = paths;
    }
    if (!scene->wf_counts.p)
        HIP_TRY(scene->wf_counts.upload(nullptr, sizeof(unsigned int) * 80));
    if (!scene->wf_done)
        HIP_TRY(hipEventCreateWithFlags(&scene->wf_done, hipEventDisableTiming));
    return SHRAY_OK;
}

// the wavefront form: one launch per bounce over queues of live paths
int launch_wavefront_view(shray_scene *scene, const FrameView &fr, const FrameView *d_view, bool all_metal, float4 *d_out, hipStream_t stream)
{
    if (const int rc = ensure_wavefront_queues(scene, (size_t)fr.width * fr.height * fr.spp))
        return rc;
    if (fr.bounce_count + 2 > 80)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "bounce_count %d is too large for the wavefront kernel", fr.bounce_count);
    if (scene->wf_pending)
        HIP_TRY(hipStreamWaitEvent(stream, scene->wf_done, 0));
    const hipError_t we = launch_wavefront(scene->view, d_view, fr, all_metal, (PathState *)scene->wf_queue0.p, (PathState *)scene->wf_queue1.p,
                                           (unsigned int *)scene->wf_counts.p, (float4 *)scene->wf_radiance.p, d_out, stream, scene->stack_levels);
    if (we != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(we));
    HIP_TRY(hipEventRecord(scene->wf_done, stream));
    scene->wf_pending = true;
    return SHRAY_OK;
}

// The stack kernel reads its FrameViews from device memory (far fewer scalar registers held, and
// spilled, than with the 480-byte view as a by-value kernel argument): `count` views travel through a
// ring of slots (pinned staging -> device, on `stream`), then one launch renders them all.
// tally / policy_frames: shray_render_counters_timed -- the instance a launch of `policy_frames` frames would run, with
// per-ray work tallies
int launch_stack_views(shray_scene *scene, const FrameView *views, int count, float4 *d_out, size_t frame_stride,
                       hipStream_t stream, DeviceCounters *tally = nullptr, int policy_frames = 0, bool tally_full_walk = false)
{
    if (views[0].total_patches == 0)
        return SHRAY_OK;
    if (!scene->batch_staging) {
        const size_t bytes = sizeof(FrameView) * kBatchSlots * SHRAY_MAX_BATCH;
        HIP_TRY(hipHostMalloc((void **)&scene->batch_staging, bytes, hipHostMallocDefault));
        HIP_TRY(scene->batch_views.upload(nullptr, bytes));
        for (int k = 0; k < kBatchSlots; k++)
            HIP_TRY(hipEventCreateWithFlags(&scene->batch_done[k], hipEventDisableTiming));
    }
    // 1. the slot.  Launch number `seq` uses slot (seq - 1) % kBatchSlots and first waits for the launch that used it before:
    // once this wait has returned, every launch up to seq - kBatchSlots is over (each was waited for by its slot's next
    // user), which is all that launch_is_over (scene_buffers.h) knows
    const unsigned long long seq = ++scene->launch_seq;
    const int slot = (int)((seq - 1) % kBatchSlots);
    if (scene->batch_pending[slot])
        HIP_TRY(hipEventSynchronize(scene->batch_done[slot]));   // rarely waits: the launch kBatchSlots launches ago
    FrameView *staged = scene->batch_staging + (size_t)slot * SHRAY_MAX_BATCH;
    FrameView *d_views = (FrameView *)scene->batch_views.p + (size_t)slot * SHRAY_MAX_BATCH;
    memcpy(staged, views, sizeof(FrameView) * (size_t)count);

    LaunchKind kind = {true, true, false, false, tally != nullptr};
    for (int k = 0; k < count; k++) {
        kind.all_plain = kind.all_plain && plain_view(views[k]);   // (the shader's debug views stay on the stack kernel's own instances)
        kind.all_metal = kind.all_metal && metal(views[k]);
    }
    kind.pair = kind.all_plain && pair_policy(scene, views, count);
    kind.deal = leaf_stage_policy(scene, policy_frames > 0 ? policy_frames : count, views[0].spp);

    // 2. heaviest patches first (dispatch_order.h): the staged views get an order and a cost buffer, or stay row-major
    bool ordered = false;
    if (const int rc = dispatch_order_attach(scene, views, count, staged, kind, seq, stream, &ordered))
        return rc;
    // 3. the view cache (view_cache.h): the staged views get their cached tables; `builds`: the entries this launch fills
    ViewBuilds builds;
    view_cache_attach(scene, views, count, staged, seq, stream, tally != nullptr, &builds);
    // 4. the staged views go up, 5. the new cache entries are filled behind them, in front of the frame kernel
    const hipError_t staged_up = hipMemcpyAsync(d_views, staged, sizeof(FrameView) * (size_t)count, hipMemcpyHostToDevice, stream);
    if (const int rc = view_cache_fill(scene, builds, views, d_views, staged_up == hipSuccess, stream))
        return rc;
    HIP_TRY(staged_up);

    // 6. the kernel
    if (scene->kernel_id == 4 && kind.all_plain && !tally && count == 1 && views[0].tile_stride == 0) {
        if (const int rc = launch_wavefront_view(scene, views[0], d_views, kind.all_metal, d_out, stream))
            return rc;
    } else {
        // (the pool kernel renders which == 0 frames)
        const hipError_t e = (scene->kernel_id == 2 && kind.all_plain && !tally)
            ? launch_pool_batch(scene->view, d_views, count, views[0], kind.all_metal, d_out, frame_stride, stream, scene->stack_levels)
            : launch_stack_batch(scene->view, d_views, count, views[0], kind.all_metal, kind.all_plain, kind.deal, d_out, frame_stride, stream,
                                 scene->stack_levels, tally, kind.pair, tally_full_walk, ordered);
        if (e != hipSuccess)
            return fail(SHRAY_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
        // 7. the shape's next permutation, behind the launch
        if (ordered)
            if (const int rc = dispatch_order_resort(scene, seq, stream))
                return rc;
    }
    // 8. the slot's event (behind the order kernel, which reads and writes the shape's buffers: "launch seq is over" covers it)
    HIP_TRY(hipEventRecord(scene->batch_done[slot], stream));
    scene->batch_pending[slot] = true;
    return SHRAY_OK;
}

int launch(shray_scene *s, const FrameView &fr_in, float4 *d_out, DeviceCounters *d_counters, hipStream_t stream)
{
    FrameView fr = fr_in;
    if (fr.total_patches == 0)
        return SHRAY_OK;
    hipError_t e;
    if (s->kernel_id != 1 && s->packed_ok && !d_counters)
        return launch_stack_views(s, &fr, 1, d_out, 0, stream);
    if (s->kernel_id == 3 && s->packed_ok && d_counters && plain_view(fr) && pair_policy(s, &fr, 1))
        return launch_stack_views(s, &fr, 1, d_out, 0, stream, d_counters, 0, true);   // the pair traversal's own counting twin
    else if (s->kernel_id == 2 && s->packed_ok && plain_view(fr))
        e = launch_pool(s->view, fr, d_out, d_counters, stream, s->stack_levels);
    else if (s->kernel_id != 1 && s->packed_ok)
        e = launch_stack(s->view, fr, d_out, d_counters, stream, s->stack_levels);
    else
        e = launch_threaded(s->view, fr, d_out, d_counters, stream);
    if (e != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    return SHRAY_OK;
}

int ensure_frame(shray_scene *scene, size_t bytes)
{
    if (scene->frame_bytes < bytes) {
        // plain allocation: a fill on the null stream would not be ordered against the kernels that write the
        // frame on other (non-blocking) streams, and every pixel is written by the render anyway
        scene->frame.release();
        scene->frame_bytes = 0;
        HIP_TRY(hipMalloc(&scene->frame.p, bytes));
        scene->frame_bytes = bytes;
    }
    if (!scene->readback_stream)
        HIP_TRY(hipStreamCreateWithFlags(&scene->readback_stream, hipStreamNonBlocking));
    return SHRAY_OK;
}

bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // pageable memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

}   // namespace

extern "C" {

int64_t shray_tile_buffer_bytes(int width, int height, const shray_tile_set *tiles) { return tile_buffer_bytes(width, height, tiles); }

int shray_render_device(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                        const shray_tile_set *tiles, void *d_rgba_out, void *hip_stream)
{
    if (!scene || !d_rgba_out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or output buffer is NULL");
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    if (!scene->view.env)
        return fail(SHRAY_ERR_NO_ENVIRONMENT, "no environment set; call shray_scene_set_environment first");
    FrameView fr;
    rc = make_frame_view(params, width, height, spp, tiles, &fr);
    if (rc)
        return rc;
    rc = use_device(scene->device);   // the scene's buffers and the stream live on its device
    if (rc)
        return rc;
    return launch(scene, fr, (float4 *)d_rgba_out, nullptr, (hipStream_t)hip_stream);
}

int shray_render_batch_device(shray_scene *scene, const shray_frame_params *params, int count, int width, int height,
                              int spp, const shray_tile_set *tiles, void *d_rgba_out, int64_t frame_stride_bytes,
                              void *hip_stream)
{
    if (!scene || !d_rgba_out || !params)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, params or output buffer is NULL");
    if (count < 1 || count > SHRAY_MAX_BATCH)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "batch of %d frames (1..%d allowed)", count, SHRAY_MAX_BATCH);
    if (!scene->view.env)
        return fail(SHRAY_ERR_NO_ENVIRONMENT, "no environment set; call shray_scene_set_environment first");
    const int64_t frame_bytes = shray_tile_buffer_bytes(width, height, tiles);
    if (frame_stride_bytes < frame_bytes || frame_stride_bytes % 16 != 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "frame_stride_bytes %lld must be a multiple of 16 and at least the %lld "
                    "bytes of one frame", (long long)frame_stride_bytes, (long long)frame_bytes);
    std::vector<FrameView> views((size_t)count);
    for (int k = 0; k < count; k++) {
        int rc = validate_params(params + k, width, height, spp);
        if (rc)
            return rc;
        rc = make_frame_view(params + k, width, height, spp, tiles, &views[k]);
        if (rc)
            return rc;
        const bool diff0 = views[0].which == 1 || views[0].which == 2, diffk = views[k].which == 1 || views[k].which == 2;
        if (diff0 != diffk)
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "frames %d and 0 of a batch disagree on differential views "
                        "(which = %d vs %d)", k, views[k].which, views[0].which);
    }
    if (const int rc = use_device(scene->device))
        return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    char *out = (char *)d_rgba_out;

    // anything but the stack kernel runs as plain consecutive launches
    if (scene->kernel_id == 1 || scene->kernel_id == 4 || !scene->packed_ok) {
        for (int k = 0; k < count; k++) {
            const int rc = launch(scene, views[k], (float4 *)(out + (size_t)k * frame_stride_bytes), nullptr, stream);
            if (rc)
                return rc;
        }
        return SHRAY_OK;
    }
    return launch_stack_views(scene, views.data(), count, (float4 *)d_rgba_out, (size_t)frame_stride_bytes / 16, stream);
}

int shray_assemble_tiles_split_device(const void *d_gathered, int world, int rank0_phases, int other_phases, int frames,
                                      int channels, int64_t rank_stride_bytes, int64_t frame_stride_bytes, int width, int height,
                                      int tile_w, int tile_h, void *d_rgba_out, void *hip_stream)
{
    if (!d_gathered || !d_rgba_out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "gathered or output buffer is NULL");
    if (world < 1 || frames < 1 || frames > 65535 || (channels != 3 && channels != 4) || width <= 0 || height <= 0 ||
        width > 65536 || height > 65535 || tile_w <= 0 || tile_h <= 0 || rank0_phases < 1 || other_phases < 1 ||
        rank0_phases > 4096 || other_phases > 4096)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "bad assemble geometry (world %d, shares %d / %d, %d frames, %d channels, %dx%d, "
                    "tiles %dx%d)", world, rank0_phases, other_phases, frames, channels, width, height, tile_w, tile_h);
    const int64_t tiles = (int64_t)((width + tile_w - 1) / tile_w) * ((height + tile_h - 1) / tile_h);
    const int64_t period = rank0_phases + (int64_t)(world - 1) * other_phases;
    int64_t most = owned_tile_count(tiles, period, 0, rank0_phases);
    for (int r = 1; r < world; r++)
        most = std::max(most, owned_tile_count(tiles, period, rank0_phases + (int64_t)(r - 1) * other_phases, other_phases));
    const int64_t frame_bytes = most * tile_w * tile_h * channels * 4;
    if (frame_stride_bytes < frame_bytes || frame_stride_bytes % 4 || rank_stride_bytes % 4 ||
        rank_stride_bytes < (int64_t)(frames - 1) * frame_stride_bytes + frame_bytes)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "strides too small: a rank's frame takes %lld bytes (frame stride %lld, "
                    "rank stride %lld)", (long long)frame_bytes, (long long)frame_stride_bytes, (long long)rank_stride_bytes);
    const hipError_t e = launch_assemble_tiles((const float *)d_gathered, (float4 *)d_rgba_out, world, rank0_phases, other_phases,
                                               frames, channels, width, height, tile_w, tile_h, (size_t)rank_stride_bytes / 4,
                                               (size_t)frame_stride_bytes / 4, (hipStream_t)hip_stream);
    if (e != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    return SHRAY_OK;
}

int shray_assemble_tiles_device(const void *d_gathered, int world, int frames, int channels, int64_t rank_stride_bytes,
                                int64_t frame_stride_bytes, int width, int height, int tile_w, int tile_h,
                                void *d_rgba_out, void *hip_stream)
{
    return shray_assemble_tiles_split_device(d_gathered, world, 1, 1, frames, channels, rank_stride_bytes, frame_stride_bytes, width,
                                             height, tile_w, tile_h, d_rgba_out, hip_stream);
}

int shray_render(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                 float *rgba_out_host)
{
    if (!scene || !rgba_out_host)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or output buffer is NULL");
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(scene->device));
    const size_t bytes = (size_t)width * height * 16;
    rc = ensure_frame(scene, bytes);
    if (rc)
        return rc;
    hipStream_t stream = scene->readback_stream;
    rc = shray_render_device(scene, params, width, height, spp, nullptr, scene->frame.p, stream);
    if (rc)
        return rc;
    // pinned destination (shray_pinned_alloc): one DMA straight into the caller's buffer; pageable: the runtime
    // stages the copy through its own pinned buffers -- the same call either way
    HIP_TRY(hipMemcpyAsync(rgba_out_host, scene->frame.p, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return SHRAY_OK;
}

int shray_render_host_async(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                            float *rgba_out_pinned, void *hip_stream)
{
    if (!scene || !rgba_out_pinned)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or output buffer is NULL");
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(scene->device));
    if (!is_pinned_host(rgba_out_pinned))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_render_host_async needs pinned host memory (shray_pinned_alloc); "
                    "use shray_render for pageable buffers");
    const size_t bytes = (size_t)width * height * 16;
    rc = ensure_frame(scene, bytes);
    if (rc)
        return rc;
    rc = shray_render_device(scene, params, width, height, spp, nullptr, scene->frame.p, hip_stream);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(rgba_out_pinned, scene->frame.p, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    return SHRAY_OK;
}

int shray_pinned_alloc(size_t bytes, void **out_ptr)
{
    if (!out_ptr || bytes == 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_pinned_alloc: NULL result pointer or zero size");
    *out_ptr = nullptr;
    HIP_TRY(hipHostMalloc(out_ptr, bytes, hipHostMallocDefault));
    return SHRAY_OK;
}

int shray_pinned_free(void *ptr)
{
    if (ptr)
        HIP_TRY(hipHostFree(ptr));
    return SHRAY_OK;
}

int shray_render_counters(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                          float *rgba_out_host, shray_counters *counters)
{
    if (!scene || !counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or counters is NULL");
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    if (!scene->view.env)
        return fail(SHRAY_ERR_NO_ENVIRONMENT, "no environment set; call shray_scene_set_environment first");
    HIP_TRY(hipSetDevice(scene->device));
    FrameView fr;
    rc = make_frame_view(params, width, height, spp, nullptr, &fr);
    if (rc)
        return rc;
    DeviceBuffer frame;
    const size_t bytes = (size_t)width * height * 16;
    HIP_TRY(frame.upload(nullptr, bytes));
    HIP_TRY(hipMemset(scene->counters.p, 0, sizeof(DeviceCounters) * kCounterShards));
    rc = launch(scene, fr, (float4 *)frame.p, (DeviceCounters *)scene->counters.p, nullptr);
    if (rc)
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    shray_counters sum = {};
    rc = sum_counter_shards((const DeviceCounters *)scene->counters.p, &sum);
    if (rc)
        return rc;
    if (rgba_out_host)
        HIP_TRY(hipMemcpy(rgba_out_host, frame.p, bytes, hipMemcpyDeviceToHost));
    sum.samples = (uint64_t)width * height * spp;
    *counters = sum;   // (the caller's counters are written only on success)
    return SHRAY_OK;
}

int shray_render_counters_timed(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                                int frames_per_launch, float *rgba_out_host, shray_counters *counters)
{
    if (!scene || !counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or counters is NULL");
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    if (frames_per_launch < 1 || frames_per_launch > SHRAY_MAX_BATCH)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "frames_per_launch %d (1..%d)", frames_per_launch, SHRAY_MAX_BATCH);
    // only the stack kernel's convergent instances have a timed form of their own; everything else is timed as it counts
    if ((scene->kernel_id != 0 && scene->kernel_id != 3 && scene->kernel_id != 4) || !scene->packed_ok || !plain_view(params->which))
        return shray_render_counters(scene, params, width, height, spp, rgba_out_host, counters);
    if (!scene->view.env)
        return fail(SHRAY_ERR_NO_ENVIRONMENT, "no environment set; call shray_scene_set_environment first");
    HIP_TRY(hipSetDevice(scene->device));
    FrameView fr;
    rc = make_frame_view(params, width, height, spp, nullptr, &fr);
    if (rc)
        return rc;
    DeviceBuffer frame;
    const size_t bytes = (size_t)width * height * 16;
    HIP_TRY(frame.upload(nullptr, bytes));
    HIP_TRY(hipMemset(scene->counters.p, 0, sizeof(DeviceCounters) * kCounterShards));
    HIP_TRY(hipDeviceSynchronize());
    rc = launch_stack_views(scene, &fr, 1, (float4 *)frame.p, 0, nullptr, (DeviceCounters *)scene->counters.p, frames_per_launch);
    if (rc)
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    rc = sum_counter_shards((const DeviceCounters *)scene->counters.p, counters);
    if (rc)
        return rc;
    counters->samples = (uint64_t)width * height * spp;
    if (rgba_out_host)
        HIP_TRY(hipMemcpy(rgba_out_host, frame.p, bytes, hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

#ifdef SHRAY_DIAGNOSTICS
// Diagnostic build only (libshray_hip_diag.so, profiles/timeline.py): renders one frame with
// the timed kernel and returns per wave 8 x uint64 {begin, end (100 MHz ticks), xcc<<32|hw_id, 0,
// node-loop iterations, leaf-loop iterations, cycles in the node loop, cycles in the leaf loop}
// (stack kernel);
// `stamps` must hold 64 * ceil(w/16) * ceil(h/16) values.
int shray_debug_timeline(shray_scene *scene, const shray_frame_params *params, int width, int height, int spp,
                         uint64_t *stamps)
{
    int rc = validate_params(params, width, height, spp);
    if (rc)
        return rc;
    FrameView fr;
    rc = make_frame_view(params, width, height, spp, nullptr, &fr);
    if (rc)
        return rc;
    const size_t nstamps = (size_t)fr.total_patches * 64;
    DeviceBuffer frame, dbg;
    HIP_TRY(frame.upload(nullptr, (size_t)width * height * 16));
    HIP_TRY(dbg.upload(nullptr, sizeof(DeviceCounters) * kCounterShards + nstamps * 8));
    shray::g_diag_plain_kernel = true;   // stamp the timed (non-counting) kernel
    // warm caches; SHRAY_DIAG_REPS back-to-back launches (about 2 s of them) let the clock settle under load before the
    // in-kernel clock is read from the last run's stamps, which are the ones returned
    const char *reps_env = getenv("SHRAY_DIAG_REPS");
    const int reps = reps_env ? std::max(1, atoi(reps_env)) : 3;
    for (int rep = 0; rep < reps; rep++) {
        rc = launch(scene, fr, (float4 *)frame.p, (DeviceCounters *)dbg.p, nullptr);
        if (rc)
            return rc;
        HIP_TRY(hipDeviceSynchronize());
    }
    shray::g_diag_plain_kernel = false;
    HIP_TRY(hipMemcpy(stamps, (char *)dbg.p + sizeof(DeviceCounters) * kCounterShards, nstamps * 8, hipMemcpyDeviceToHost));
    return SHRAY_OK;
}
#endif

int shray_scene_dispatch_order(shray_scene *scene, uint32_t *order_out, uint32_t capacity, uint32_t *count_out)
{
    if (!scene || !count_out || (capacity && !order_out))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, count_out or order_out is NULL");
    HIP_TRY(hipSetDevice(scene->device));
    *count_out = 0;
    if (scene->dispatch_last < 0)
        return SHRAY_OK;
    DispatchOrder &d = scene->dispatch[scene->dispatch_last];
    HIP_TRY(hipDeviceSynchronize());
    if (d.pending_count > 0) {
        d.current = d.written;
        d.pending_count = 0;
    }
    if (d.current < 0 || d.n == 0)
        return SHRAY_OK;
    const uint32_t copy = capacity < d.n ? capacity : d.n;
    if (copy)
        HIP_TRY(hipMemcpy(order_out, (const uint32_t *)d.ring.p + (size_t)d.current * d.n, (size_t)copy * 4, hipMemcpyDeviceToHost));
    *count_out = d.n;
    return SHRAY_OK;
}

}   // extern "C"
