// capi.hip -- the parts of include/shader_ray_hip.h that belong to no mechanism of their own: the per-thread error string,
// device count and selection, the frame-parameter defaults, the environment upload, a scene's destruction and kernel choice,
// what the client libraries read of a scene (scene_access_internal.h), and the self-tests.  Scenes are made in
// scene_create.hip and rendered from render_api.hip (with dispatch_order.hip and view_cache.hip); struct shray_scene is
// scene_internal.h's.  Host code only: the kernels live in kernel_*.hip and, for scene creation, in scene_create.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "error_internal.h"
#include "frame_params_defaults.h"
#include "frame_view_host.h"
#include "launch.h"
#include "packed_layout.h"
#include "scene_access_internal.h"
#include "scene_internal.h"
#include "shader_ray_hip.h"
#include "view_cache.h"

using namespace shray;

namespace {

thread_local std::string g_error;

}   // namespace

// every error of the library and of its clients (error_internal.h) ends here
extern "C" int shrayi_fail(int code, const char *message)
{
    g_error = message;
    return code;
}

extern "C" {

int shray_abi_version(void) { return SHRAY_ABI_VERSION; }

const char *shray_last_error(void) { return g_error.c_str(); }

int shray_device_count(int *count)
{
    if (!count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        *count = 0;
        return fail(SHRAY_ERR_NO_DEVICE, "no HIP device is visible");
    }
    *count = n;
    return SHRAY_OK;
}

int shray_set_device(int device_index)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SHRAY_ERR_NO_DEVICE, "no HIP device is visible");
    if (device_index < 0 || device_index >= n)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "device %d out of range [0, %d)", device_index, n);
    HIP_TRY(hipSetDevice(device_index));
    return SHRAY_OK;
}

void shray_frame_params_init(shray_frame_params *params)
{
    if (params)
        shray_frame_params_defaults(params);
}

// GL's conversion of a float to 8-bit normalized fixed point and back (GL 3.1 section 2.1.5): clamp to [0, 1],
// c = floor(255 f + 0.5), stored value c / 255; NaN stores 0
static float through_unorm8(float f)
{
    const float clamped = !(f > 0.0f) ? 0.0f : (f > 1.0f ? 1.0f : f);
    return floorf(clamped * 255.0f + 0.5f) / 255.0f;
}

int shray_scene_set_environment(shray_scene *scene, const float *rgb, int width, int height)
{
    return shray_scene_set_environment_storage(scene, rgb, width, height, SHRAY_ENV_FLOAT32);
}

int shray_scene_set_environment_storage(shray_scene *scene, const float *rgb, int width, int height, int storage)
{
    if (!scene || !rgb || width <= 0 || height <= 0 || width > 32768 || height > 32768)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "bad environment (%p, %d x %d)", (const void *)rgb, width, height);
    if (storage != SHRAY_ENV_FLOAT32 && storage != SHRAY_ENV_UNORM8)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "environment storage %d (SHRAY_ENV_FLOAT32 or SHRAY_ENV_UNORM8)", storage);
    HIP_TRY(hipSetDevice(scene->device));
    // level 0 followed by its mip chain (2x2 box filter, ((a+b)+(c+d))*0.25, dimensions max(1, n/2)),
    // the pyramid the reference asks GL for with glGenerateMipmap (ray.cpp:509); only the which == 1
    // view reads levels above 0
    std::vector<float> pyramid(rgb, rgb + (size_t)width * height * 3);
    if (storage == SHRAY_ENV_UNORM8)
        for (float &texel : pyramid)
            texel = through_unorm8(texel);
    SceneView &v = scene->view;
    v.mip_levels = 0;
    size_t level_start = 0;
    int w = width, h = height;
    for (;;) {
        v.mip_offset[v.mip_levels] = (uint32_t)level_start;
        v.mip_w[v.mip_levels] = w;
        v.mip_h[v.mip_levels] = h;
        v.mip_levels++;
        if ((w == 1 && h == 1) || v.mip_levels == 16)
            break;
        const int nw = std::max(1, w / 2), nh = std::max(1, h / 2);
        const size_t next_start = pyramid.size();
        pyramid.resize(next_start + (size_t)nw * nh * 3);
        const float *src = pyramid.data() + level_start;
        float *dst = pyramid.data() + next_start;
        for (int j = 0; j < nh; j++)
            for (int i = 0; i < nw; i++) {
                const int i0 = std::min(2 * i, w - 1), i1 = std::min(2 * i + 1, w - 1);
                const int j0 = std::min(2 * j, h - 1), j1 = std::min(2 * j + 1, h - 1);
                for (int c = 0; c < 3; c++) {
                    const float a = src[3 * ((size_t)j0 * w + i0) + c], b = src[3 * ((size_t)j0 * w + i1) + c];
                    const float cc = src[3 * ((size_t)j1 * w + i0) + c], d = src[3 * ((size_t)j1 * w + i1) + c];
                    const float mean = ((a + b) + (cc + d)) * 0.25f;
                    dst[3 * ((size_t)j * nw + i) + c] = storage == SHRAY_ENV_UNORM8 ? through_unorm8(mean) : mean;   // every level is stored
                }
            }
        level_start = next_start;
        w = nw;
        h = nh;
    }
    // the view cache's entries hold lookups in the old environment: their keys no longer match anything
    scene->env_generation++;
    view_cache_invalidate(scene);
    HIP_TRY(scene->env.upload(pyramid.data(), pyramid.size() * sizeof(float)));
    scene->view.env = (const float *)scene->env.p;
    scene->view.env_w = width;
    scene->view.env_h = height;
    return SHRAY_OK;
}

int shray_scene_destroy(shray_scene *scene)
{
    if (!scene)
        return SHRAY_OK;
    (void)hipSetDevice(scene->device);
    delete scene;
    return SHRAY_OK;
}

int shray_scene_device(const shray_scene *scene, int *device_index)
{
    if (!scene || !device_index)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene or device_index is NULL");
    *device_index = scene->device;
    return SHRAY_OK;
}

int shrayi_scene_query_view(const shray_scene *scene, ShrayQueryScene *out)
{
    if (!scene || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    out->view = scene->view;
    out->stack_levels = scene->stack_levels;
    out->packed_ok = scene->packed_ok;
    out->kernel_id = scene->kernel_id;
    out->device = scene->device;
    return SHRAY_OK;
}

int shrayi_scene_refit_view(shray_scene *scene, ShrayRefitScene *out)
{
    if (!scene || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    const SceneView &v = scene->view;
    out->positions = (float *)scene->positions.p;
    out->normals32 = (float *)scene->normals32.p;
    out->normals16 = (uint16_t *)scene->normals16.p;
    out->boxmin = (float *)scene->boxmin.p;
    out->boxmax = (float *)scene->boxmax.p;
    out->packed_nodes = scene->packed_ok ? scene->packed_nodes.p : nullptr;
    out->packed_tris = scene->packed_ok ? scene->packed_tris.p : nullptr;
    out->pair_nodes = scene->packed_ok ? scene->pair_nodes.p : nullptr;
    out->flat_of_packed = scene->packed_ok ? (const int32_t *)scene->flat_of_packed.p : nullptr;
    out->node_count = v.group_count;
    out->triangle_count = v.triangle_count;
    out->packed_root = v.packed_root >> (kNodeShift - kNodeNameShift);
    out->exact_div_ok = v.exact_div_ok;
    out->packed_ok = scene->packed_ok;
    out->device = scene->device;
    out->state = &scene->refit_state;
    return SHRAY_OK;
}

int shrayi_scene_point_state(shray_scene *scene, std::shared_ptr<void> **out)
{
    if (!scene || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    *out = &scene->point_state;
    return SHRAY_OK;
}

int shrayi_scene_sdf_state(shray_scene *scene, std::shared_ptr<void> **out, uint64_t *generation)
{
    if (!scene || !out || !generation)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    *out = &scene->sdf_state;
    *generation = scene->geometry_generation;
    return SHRAY_OK;
}

int shrayi_scene_winding_state(shray_scene *scene, std::shared_ptr<void> **out, uint64_t *generation)
{
    if (!scene || !out || !generation)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    *out = &scene->winding_state;
    *generation = scene->geometry_generation;
    return SHRAY_OK;
}

int shrayi_scene_geometry_changed(shray_scene *scene)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    scene->geometry_generation++;
    return SHRAY_OK;
}

int shrayi_scene_set_exact_div_ok(shray_scene *scene, uint32_t ok)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    scene->view.exact_div_ok = ok ? 1u : 0u;
    return SHRAY_OK;
}

int shrayi_frame_view(const shray_frame_params *params, int width, int height, FrameView *out)
{
    const int rc = validate_params(params, width, height, 1);
    return rc ? rc : make_frame_view(params, width, height, 1, nullptr, out);
}

int shray_scene_set_kernel(shray_scene *scene, int kernel_id)
{
    if (!scene || kernel_id < 0 || kernel_id > 4)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "kernel id %d (0 = stack, 1 = threaded, 2 = pool, 3 = stack with pair turns, 4 = wavefront)",
                    kernel_id);
    if (kernel_id != 1 && !scene->packed_ok)
        return fail(SHRAY_ERR_BAD_TREE, "the scene's hit/miss tables are not a canonical threaded tree; only the "
                    "literal threaded kernel (1) can run it");
    scene->kernel_id = kernel_id;
    return SHRAY_OK;
}

int shray_selftest_division(uint64_t pairs, uint64_t seed, uint64_t *mismatches)
{
    if (!mismatches)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "mismatches is NULL");
    DeviceBuffer count;
    HIP_TRY(count.upload(nullptr, sizeof(unsigned long long)));
    hipError_t e = shray::launch_division_selftest(pairs, seed, (unsigned long long *)count.p, nullptr);
    if (e != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "self-test launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long n = 0;
    HIP_TRY(hipMemcpy(&n, count.p, sizeof(n), hipMemcpyDeviceToHost));
    *mismatches = n;
    return SHRAY_OK;
}

int shray_selftest_reciprocal(uint64_t *mismatches)
{
    if (!mismatches)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "mismatches is NULL");
    DeviceBuffer count;
    HIP_TRY(count.upload(nullptr, sizeof(unsigned long long)));
    hipError_t e = shray::launch_reciprocal_selftest((unsigned long long *)count.p, nullptr);
    if (e != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "self-test launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long n = 0;
    HIP_TRY(hipMemcpy(&n, count.p, sizeof(n), hipMemcpyDeviceToHost));
    *mismatches = n;
    return SHRAY_OK;
}

int shray_probe_vector_cache(uint32_t records, uint32_t spread, uint32_t visits_per_lane, uint32_t waves, uint64_t lane_mask, int bytes_per_lane,
                             double *seconds, uint64_t *bytes_loaded)
{
    if (!seconds || !bytes_loaded)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "seconds or bytes_loaded is NULL");
    auto power_of_two = [](uint32_t v) { return v != 0 && (v & (v - 1)) == 0; };
    const uint32_t runs = spread & 0x80000000u;
    spread &= 0x7fffffffu;
    if (!power_of_two(records) || !power_of_two(spread) || spread > records || records > (1u << 26) || visits_per_lane == 0 ||
        visits_per_lane % 8 != 0 || waves == 0 || waves > (1u << 24) ||
        !(bytes_per_lane == 32 || bytes_per_lane == 16 || bytes_per_lane == 12 || bytes_per_lane == 8 || bytes_per_lane == 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "shray_probe_vector_cache: records and spread are powers of two (spread <= records <= 2^26), "
                    "visits_per_lane a multiple of 8, waves 1..2^24, bytes_per_lane 32, 16, 12, 8 or 4");
    DeviceBuffer table, out;
    HIP_TRY(table.upload(nullptr, (size_t)records * 32));
    HIP_TRY(out.upload(nullptr, (size_t)waves * 64 * 4));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    float ms = 0.0f;
    hipError_t e = hipSuccess;
    for (int pass = 0; pass < 2 && e == hipSuccess; pass++) {      // the first pass warms the caches and the clock
        (void)hipEventRecord(a, nullptr);
        e = shray::launch_vector_cache_probe((const float4 *)table.p, records, spread | runs, visits_per_lane, waves, (unsigned long long)lane_mask, bytes_per_lane, (float *)out.p, nullptr);
        (void)hipEventRecord(b, nullptr);
        if (e == hipSuccess)
            e = hipEventSynchronize(b);
        if (e == hipSuccess)
            e = hipEventElapsedTime(&ms, a, b);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (e != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "vector-cache probe failed: %s", hipGetErrorString(e));
    *seconds = (double)ms * 1e-3;
    *bytes_loaded = (uint64_t)waves * (uint64_t)__builtin_popcountll(lane_mask) * (uint64_t)visits_per_lane * (uint64_t)bytes_per_lane;
    return SHRAY_OK;
}

}   // extern "C"
