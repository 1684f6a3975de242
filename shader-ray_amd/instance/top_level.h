// top_level.h -- what the kernels that walk an instance set's top level share (instance.hip: closest and any hit;
// instance_multihit/instance_multihit.hip: all hits): the node and record layout, a lane's widened slab test of a top-level
// box, the object ray (include/shader_ray_instance.h), and the accessors through which another library reads a set's device
// arrays and its forward maps (instance_point/instance_point.hip: closest points).  Internal to the libraries; no kernel is
// defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"
#include "shader_ray_instance.h"
#include "trace_common.h"

namespace {

using namespace shray;

constexpr int kTopStack = 32;              // per-wave top-level stack entries: the depth is at most ceil(log2 2^20) = 20
constexpr uint32_t kLeafBit = 0x80000000u; // a node link: leaf | instance, or axis << 29 | first child (the second follows it)

// A top-level node, two float4: (lo.xyz, margin factor k) and (hi.xyz, link bits).  A lane widens the box by k * |P|inf more.
struct TopNode {
    float lo[3], k;
    float hi[3];
    uint32_t link;
};
static_assert(sizeof(TopNode) == 32, "two float4");

// one lane's slab test of a top-level box over [0, limit], widened by `pad`; a NaN quotient (0 * inf at a plane) enters
__device__ __forceinline__ bool enters_box(const float4 &a, const float4 &b, const V3 &P, const V3 &D, float pad, float limit)
{
    float tn = 0.0f, tf = limit;
    const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z}, p[3] = {P.x, P.y, P.z}, d[3] = {D.x, D.y, D.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q0 = ((lo[c] - pad) - p[c]) / d[c], q1 = ((hi[c] + pad) - p[c]) / d[c];
        if (q0 == q0 && q1 == q1) {
            tn = fmaxf(tn, fminf(q0, q1));
            tf = fminf(tf, fmaxf(q0, q1));
        }
    }
    return tn <= tf;
}

// row r of W applied to v (w: also add the translation): the products of nonzero entries only, left to right
__device__ __forceinline__ float object_row(const float4 &row, const V3 &v, bool w)
{
    float acc = 0.0f;
    bool any = false;
    const float m[3] = {row.x, row.y, row.z}, x[3] = {v.x, v.y, v.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (m[c] != 0.0f) {
            const float prod = m[c] * x[c];
            acc = any ? acc + prod : prod;
            any = true;
        }
    }
    if (w && row.w != 0.0f)
        acc = any ? acc + row.w : row.w;
    return acc;
}

}   // namespace

// A set's device arrays as a query's launch reads them, and its member scenes.  The pointers are device memory of `device`
// and stay the set's own until it is destroyed or updated on the host (a device update rewrites them in place, stream-ordered).
struct ShrayInstanceSetDevice {
    const void *nodes;             // TopNode[2 count - 1], the root first
    const void *records;           // float4[count][4]: W's three rows, then (scene slot bits, 0, 0, 0)
    const void *views;             // shray::SceneView[scene_count], by scene slot
    shray_scene *const *scenes;    // host array [scene_count]: the distinct member scenes by scene slot
    int32_t count, scene_count;
    int device;
};

// Not in the header: for libshray_instance_multihit.so.  Host-only; waits for nothing and touches no device.
extern "C" int shrayi_instance_set_device_arrays(const shray_instance_set *set, ShrayInstanceSetDevice *out);

// Not in the header: for libshray_instance_point.so.  The set's current object_to_world floats on its device, float
// [count][12], for a launch enqueued on `hip_stream` after this call (an upload that is due is staged on that stream).
// Host-only; makes the set's device current and waits for nothing.
extern "C" int shrayi_instance_set_forward_maps(shray_instance_set *set, void *hip_stream, const float **d_maps);
