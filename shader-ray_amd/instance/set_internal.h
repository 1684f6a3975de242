// set_internal.h -- what libshray_instance.so's three units share: the set itself (instance_set.hip builds and owns it,
// instance_update.hip rebuilds it on the device, instance.hip walks it) and the transform and box arithmetic that the host
// build and the device update both run.  Internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "client_internal.h"
#include "shader_ray_instance.h"
#include "top_level.h"

// A named namespace: shray_instance_set's members must be the same types in every unit that sees the struct.
namespace shray_set {

using namespace shray;

// The cull's margin factor: 128 ulps of 1 times the instance's condition ||A||inf * ||W||inf
constexpr double kMarginUlps = 128.0 / 16777216.0;

// What a launch reads besides the rays: every pointer is __restrict__ in the kernel's arguments, so that the views come in
// by scalar loads (the traversal's inline asm takes their packed-array pointers as "s" operands)
struct SetDevice {
    TopNode *nodes = nullptr;     // [node_count], the root first
    float4 *records = nullptr;    // [count][4]: W's three rows, then (scene slot bits, 0, 0, 0)
    SceneView *views = nullptr;   // [distinct scenes]
};

// max and min as std::max / std::min take them: the first argument on a tie
__host__ __device__ inline double dmax(double a, double b) { return (a < b) ? b : a; }
__host__ __device__ inline double dmin(double a, double b) { return (b < a) ? b : a; }

// the neighbouring floats of a float that is not NaN, as std::nextafter(f, -inf) and std::nextafter(f, +inf) give them
__host__ __device__ inline float next_down(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    u = f == 0.0f ? 0x80000001u : (u >> 31) ? u + 1u : u - 1u;
    memcpy(&f, &u, 4);
    return f;
}
__host__ __device__ inline float next_up(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    u = f == 0.0f ? 0x00000001u : (u >> 31) ? u - 1u : u + 1u;
    memcpy(&f, &u, 4);
    return f;
}

// the float nearest x on its side: rounds a box's low corner down and its high corner up
__host__ __device__ inline float round_down(double x)
{
    float f = (float)x;
    if ((double)f > x)
        f = next_down(f);
    return f;
}
__host__ __device__ inline float round_up(double x)
{
    float f = (float)x;
    if ((double)f < x)
        f = next_up(f);
    return f;
}

// What a set is made of, built in full before it replaces anything (a failed create or update changes nothing).
struct Prepared {
    std::vector<float> object_to_world, world_to_object;   // count * 12
    std::vector<TopNode> nodes;
    std::vector<float4> records;
    std::vector<SceneView> views;
    int stack_levels = 0;
    int device = -1;
};

struct BoxRef {
    double lo[3], hi[3], centre[3];
    double k;
};

// W = the float rounding of the double inverse of object_to_world; false for a singular or non-finite map.  The host update
// and the device update (iu_instances) run this one function: their W and condition are the same bits.
__host__ __device__ inline bool invert(const float *m, float *out, double *condition)
{
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(m[j]))
            return false;
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double co[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
                          d * h - e * g, b * g - a * h, a * e - b * d};
    const double det = a * co[0] + b * co[3] + c * co[6];
    if (det == 0.0 || !std::isfinite(det))
        return false;
    const double t[3] = {m[3], m[7], m[11]};
    double norm_a = 0.0, norm_w = 0.0;
    for (int r = 0; r < 3; ++r) {
        double wt = 0.0, row_w = 0.0;
        for (int col = 0; col < 3; ++col) {
            const double inv = co[3 * r + col] / det;
            out[4 * r + col] = (float)inv;
            wt -= inv * t[col];
            row_w += fabs((double)out[4 * r + col]);
        }
        out[4 * r + 3] = (float)wt;
        norm_a = dmax(norm_a, fabs((double)m[4 * r]) + fabs((double)m[4 * r + 1]) + fabs((double)m[4 * r + 2]));
        norm_w = dmax(norm_w, row_w);
    }
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(out[j]))
            return false;
    *condition = norm_a * norm_w;
    return std::isfinite(*condition);
}

// the world box: the root box rb (lo xyz, hi xyz)'s 8 corners through object_to_world in double, widened by the margin
// (DESIGN.md section 10), its margin factor k and its centre; shared by the host and the device update like invert
__host__ __device__ inline void place_box(const float *m, const float *rb, double condition, BoxRef &b)
{
    for (int c = 0; c < 3; ++c) {
        b.lo[c] = INFINITY;
        b.hi[c] = -INFINITY;
    }
    for (int corner = 0; corner < 8; ++corner) {
        const double x[3] = {rb[(corner & 1) ? 3 : 0], rb[(corner & 2) ? 4 : 1], rb[(corner & 4) ? 5 : 2]};
        for (int r = 0; r < 3; ++r) {
            const double y = (double)m[4 * r] * x[0] + (double)m[4 * r + 1] * x[1] + (double)m[4 * r + 2] * x[2] + (double)m[4 * r + 3];
            b.lo[r] = dmin(b.lo[r], y);
            b.hi[r] = dmax(b.hi[r], y);
        }
    }
    // k * (|world box|inf + |b|inf); each lane adds k * |P|inf
    double box_reach = 0.0;
    for (int c = 0; c < 3; ++c)
        box_reach = dmax(dmax(box_reach, fabs(b.lo[c])), fabs(b.hi[c]));
    const double reach = box_reach + dmax(dmax(fabs((double)m[3]), fabs((double)m[7])), fabs((double)m[11]));
    b.k = kMarginUlps * condition;
    for (int c = 0; c < 3; ++c) {
        b.lo[c] -= b.k * reach;
        b.hi[c] += b.k * reach;
        b.centre[c] = 0.5 * (b.lo[c] + b.hi[c]);
    }
}

// pinned host memory a copy reads from, free again once `copied` has completed
struct Staging {
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
};

// waits for every copy of `staging` and frees its pinned memory
inline void release(std::vector<Staging> &staging)
{
    for (Staging &s : staging) {
        if (s.copied)
            (void)hipEventSynchronize(s.copied);
        if (s.host)
            (void)hipHostFree(s.host);
        if (s.copied)
            (void)hipEventDestroy(s.copied);
    }
    staging.clear();
}

// The device copy of the set's current object-to-world maps, float [12 n]: what the device update keeps between its calls and
// what a query that needs the forward maps reads (shrayi_instance_set_forward_maps).  Allocated by whichever comes first; a
// host update leaves it behind the host copy (`stale`), and the next reader stages the upload on its own stream.  `uploaded`
// is recorded after that copy, so that a reader on another stream can wait for it without the host.
struct ForwardMaps {
    DeviceBuffer transforms;
    bool stale = true;                        // behind the host copy: before the first use, and after a host update
    std::vector<Staging> staging;
    hipEvent_t uploaded = nullptr;
    bool recorded = false;
    ~ForwardMaps()
    {
        release(staging);
        if (uploaded)
            (void)hipEventDestroy(uploaded);
    }
};

// What the device update keeps per set: its scratch (sized by the set's count, allocated by the first device update) and what
// it last uploaded.  Defined here, not beside its kernels: the set's accessors wait on `finished` and read `enqueued`.
struct DeviceUpdate {
    uint32_t n = 0;
    int depth = 0;                            // levels of splits: ceil(log2 n)
    std::vector<shray_scene *> distinct;      // the member scenes in scene-slot order (the host's: first appearance)
    std::vector<SceneView> staged;            // what `views` holds, once views_staged
    bool views_staged = false;
    DeviceBuffer words;                       // int32 [0]: the refusal word, [1]: the status of the last update
    DeviceBuffer records, leaves, nodes, centres, keys, sorted_keys, ids, lists[2], left_of, flags, offsets, views, temp;
    size_t temp_bytes = 0;
    std::vector<Staging> staging;
    hipEvent_t finished = nullptr;            // recorded after the last device update's commit
    bool enqueued = false;
    ~DeviceUpdate()
    {
        release(staging);
        if (finished)
            (void)hipEventDestroy(finished);
    }
};

// instance_set.hip's: host memory to device memory at `dst` on `stream` through pinned memory, and the device copy of the
// set's object-to-world maps, current for work enqueued on `stream` after the call (neither waits for the host)
int stage(std::vector<Staging> &staging, hipStream_t stream, void *dst, const void *src, size_t bytes);
int current_maps(shray_instance_set *set, hipStream_t stream);

}   // namespace shray_set

struct shray_instance_set {
    std::vector<shray_scene *> scenes;
    std::vector<shray_scene *> distinct;    // the member scenes by scene slot (prepare's: first appearance)
    shray_set::Prepared host;
    shray_set::SetDevice dev;
    std::unique_ptr<shray_set::DeviceUpdate> update;   // the device update's state, once one was made
    std::unique_ptr<shray_set::ForwardMaps> maps;      // the device copy of object_to_world, once something asked for it
    bool host_stale = false;                // host.object_to_world / world_to_object may be behind a device update
};
