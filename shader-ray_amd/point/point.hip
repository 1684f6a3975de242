// point.hip -- include/shader_ray_point.h: the nearest point of a resident scene's surface to each caller-supplied point.
//
// The walk (one lane per point over the packed tree, nearest child first) is point_walk.h, which
// libshray_sdf.so compiles too.  This library is built apart from libshray_hip.so, so the renderer's code objects do not
// change.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "client_internal.h"
#include "device_types.h"
#include "error_internal.h"
#include "point_walk.h"
#include "scene_access_internal.h"
#include "shader_ray_point.h"

using namespace shray;

namespace {

int closest_device(shray_scene *scene, const shray_point *d_points, int64_t count, shray_closest *d_out, hipStream_t stream,
                   DeviceCounters *d_counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!scene || !d_points || !d_out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, points or out is NULL");
    if (!aligned(d_points, 16) || !aligned(d_out, 16))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "point and record buffers must be 16-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    const int rc = enter_walkable_scene(scene, &q, &height);
    return rc ? rc : enqueue_closest(q, height, d_points, (uint64_t)count, d_out, stream, d_counters);
}

// the blocking forms: the points to the device, the query on the null stream, the records (and tallies) back
int closest_host(shray_scene *scene, const shray_point *points, int64_t count, shray_closest *out, shray_counters *counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!scene || !points || (!out && !counters))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene, points or out is NULL");
    if (counters) {
        memset(counters, 0, sizeof(*counters));
        counters->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    ShrayQueryScene q;
    int height = 0;
    const int rc = enter_walkable_scene(scene, &q, &height);   // (the errors of a scene come before any allocation)
    if (rc)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{out, n * sizeof(shray_closest)}}, counters,
                        [&](DeviceBuffer *d_points, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return closest_device(scene, d_points->as<const shray_point>(), count, d_out->as<shray_closest>(), nullptr, shards);
                        });
}

}   // namespace

static_assert(sizeof(shray_point) == 16, "shray_point is 16 bytes");
static_assert(sizeof(shray_closest) == 32, "shray_closest is 32 bytes");

extern "C" {

int shray_closest_points_device(shray_scene *scene, const shray_point *d_points, int64_t count, shray_closest *d_out,
                                void *hip_stream)
{
    return closest_device(scene, d_points, count, d_out, (hipStream_t)hip_stream, nullptr);
}

int shray_closest_points(shray_scene *scene, const shray_point *points, int64_t count, shray_closest *out)
{
    if (!out && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "out is NULL");
    return closest_host(scene, points, count, out, nullptr);
}

int shray_closest_points_counters(shray_scene *scene, const shray_point *points, int64_t count, shray_closest *out,
                                  shray_counters *counters)
{
    if (!counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return closest_host(scene, points, count, out, counters);
}

}   // extern "C"
