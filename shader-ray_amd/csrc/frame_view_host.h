// frame_view_host.h -- from a caller's shray_frame_params, frame size and tile set to the FrameView a launch carries: the
// checks, the tiling arithmetic and the size of the buffer a tile set's frame takes.  Shared by render_api.hip and capi.hip
// (shrayi_frame_view).  Host-only, internal to the library.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "device_types.h"
#include "error_internal.h"
#include "shader_ray_hip.h"

// 1: multi-sample frames run a pixel's samples in neighbouring lanes (uniform_driver.h); 0: one lane per pixel
// at most 2^5 = 32 lanes per pixel: plaster 64 spp 16.38 / 15.83 / 16.26 ms with up to 64 / 32 / 16 (profiles/sample_lanes_probe.sh)
#ifndef SHRAY_SAMPLE_LANES_LOG2_MAX
#define SHRAY_SAMPLE_LANES_LOG2_MAX 5
#endif

namespace shray {

inline int validate_params(const shray_frame_params *p, int width, int height, int spp)
{
    if (!p)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "frame params are NULL");
    if (p->struct_size != sizeof(shray_frame_params))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_frame_params.struct_size is %u, this library expects %zu",
                    p->struct_size, sizeof(shray_frame_params));
    if (width <= 0 || height <= 0 || spp <= 0 || width > 65536 || height > 65536 || spp > (1 << 20))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "bad frame geometry %dx%d, %d spp", width, height, spp);
    if ((p->which == 3 || p->which == 5) && spp != 1)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "which = %d is a per-pixel view; spp must be 1", p->which);
    if (p->bounce_count < 0 || p->bounce_count > 64 || p->max_bvh_iterations < 1 || p->max_bvh_iterations > (1 << 24) ||
        p->max_leaf_tests < 0 || p->max_leaf_tests > (1 << 24))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shader constants out of range (bounce_count %d, max_bvh_iterations %d, "
                    "max_leaf_tests %d)", p->bounce_count, p->max_bvh_iterations, p->max_leaf_tests);
    return SHRAY_OK;
}

// tiles t < total with phase <= t % stride < phase + count
inline int64_t owned_tile_count(int64_t total, int64_t stride, int64_t phase, int64_t count)
{
    return total / stride * count + std::min(count, std::max<int64_t>(0, total % stride - phase));
}

inline int make_frame_view(const shray_frame_params *p, int width, int height, int spp, const shray_tile_set *tiles,
                           FrameView *fr)
{
    memset(fr, 0, sizeof(*fr));
    memcpy(fr->camera_matrix, p->camera_matrix, 64);
    memcpy(fr->camera_normal_matrix, p->camera_normal_matrix, 64);
    memcpy(fr->object_matrix, p->object_matrix, 64);
    memcpy(fr->object_normal_matrix, p->object_normal_matrix, 64);
    memcpy(fr->object_normal_inverse, p->object_normal_inverse, 64);
    fr->image_plane_width = p->image_plane_width;
    fr->aspect = p->aspect;
    memcpy(fr->light_dir, p->light_dir, 12);
    memcpy(fr->specular_color, p->specular_color, 12);
    memcpy(fr->diffuse_color, p->diffuse_color, 12);
    fr->bounce_count = p->bounce_count;
    fr->max_bvh_iterations = p->max_bvh_iterations;
    fr->max_leaf_tests = p->max_leaf_tests;
    fr->cast_shadows = p->cast_shadows;
    fr->tonemap = p->tonemap;
    fr->normals_fp16 = p->normals_fp16;
    fr->which = p->which;
    memcpy(fr->right, p->right, 12);
    memcpy(fr->up, p->up, 12);
    fr->width = width;
    fr->height = height;
    fr->spp = spp;
    // lanes per pixel of a multi-sample frame (uniform_driver.h): the largest power of two <= min(spp, 32), as a
    // block of 2^x by 2^y neighbouring lanes of the wave's 8x8 lane grid
    {
        int log_g = 0;
        while (log_g < SHRAY_SAMPLE_LANES_LOG2_MAX && (2 << log_g) <= spp)
            log_g++;
        fr->sample_log_x = (uint32_t)((log_g + 1) / 2);
        fr->sample_log_y = (uint32_t)(log_g / 2);
    }

    const bool tiled = tiles && tiles->tile_stride > 0;
    if (!tiled) {
        fr->tile_stride = 0;
        fr->patches_x = (width + 15) / 16;
        fr->patches_per_unit = fr->patches_x * ((height + 15) / 16);
        fr->total_patches = (uint32_t)fr->patches_per_unit;
        return SHRAY_OK;
    }
    const int phase_count = tiles->tile_phase_count > 0 ? tiles->tile_phase_count : 1;
    if (tiles->tile_w <= 0 || tiles->tile_h <= 0 || tiles->tile_w % 16 || tiles->tile_h % 16 ||
        tiles->tile_phase < 0 || tiles->tile_phase_count < 0 || tiles->tile_phase + phase_count > tiles->tile_stride)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "tile set {%d x %d, stride %d, phase %d, count %d}: tile sizes must be positive "
                    "multiples of 16 and 0 <= phase, phase + count <= stride", tiles->tile_w, tiles->tile_h, tiles->tile_stride,
                    tiles->tile_phase, phase_count);
    fr->tile_w = tiles->tile_w;
    fr->tile_h = tiles->tile_h;
    fr->tile_stride = tiles->tile_stride;
    fr->tile_phase = tiles->tile_phase;
    fr->tile_phase_count = phase_count;
    fr->tiles_x = (width + tiles->tile_w - 1) / tiles->tile_w;
    const int tiles_y = (height + tiles->tile_h - 1) / tiles->tile_h;
    fr->owned_tiles = (int32_t)owned_tile_count((int64_t)fr->tiles_x * tiles_y, tiles->tile_stride, tiles->tile_phase, phase_count);
    fr->patches_x = tiles->tile_w / 16;
    fr->patches_per_unit = fr->patches_x * (tiles->tile_h / 16);
    fr->total_patches = (uint32_t)fr->owned_tiles * (uint32_t)fr->patches_per_unit;
    return SHRAY_OK;
}

// bytes of the RGBA32F buffer one frame of `tiles` takes (the whole frame without a tile set); 0: a malformed request
inline int64_t tile_buffer_bytes(int width, int height, const shray_tile_set *tiles)
{
    if (width <= 0 || height <= 0)
        return 0;
    if (!tiles || tiles->tile_stride <= 0)
        return (int64_t)width * height * 16;
    const int phase_count = tiles->tile_phase_count > 0 ? tiles->tile_phase_count : 1;
    if (tiles->tile_w <= 0 || tiles->tile_h <= 0 || tiles->tile_phase < 0 || tiles->tile_phase_count < 0 ||
        tiles->tile_phase + phase_count > tiles->tile_stride)
        return 0;
    const int64_t tx = (width + tiles->tile_w - 1) / tiles->tile_w, ty = (height + tiles->tile_h - 1) / tiles->tile_h;
    return owned_tile_count(tx * ty, tiles->tile_stride, tiles->tile_phase, phase_count) * tiles->tile_w * tiles->tile_h * 16;
}

}   // namespace shray
