// top_level.h -- the walk of an instance set's top level and what its six callers share (instance.hip: closest and any hit;
// instance_multihit/: all hits; instance_point/, instance_near/, instance_overlap/, instance_intersect/: points, boxes, triangles).  walk_top_level
// is the only loop over TopNodes in device code; DESIGN.md sections 10, 16 and 20 argue it.  Beside it: the node and record
// layout, a lane's widened slab test, the object ray (include/shader_ray_instance.h), a leaf's SceneView, and the accessors
// through which another library reads a set's device arrays and forward maps.  Internal to the libraries; no kernel here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"
#include "shader_ray_instance.h"
#include "trace_common.h"

namespace shray {

// A top-level node, two float4: (lo.xyz, margin factor k) and (hi.xyz, link bits).  A lane widens the box by k * |P|inf more.
struct TopNode {
    float lo[3], k;
    float hi[3];
    uint32_t link;
};
static_assert(sizeof(TopNode) == 32, "two float4");

}   // namespace shray

namespace {

using namespace shray;

constexpr int kTopStack = 32;              // per-wave top-level stack entries: the depth is at most ceil(log2 2^20) = 20
constexpr uint32_t kLeafBit = 0x80000000u; // a node link: leaf | instance, or axis << 29 | first child (the second follows it)

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

// the object ray of a world ray under a record's three rows of W
__device__ __forceinline__ void object_ray(const float4 *rec, const V3 &P, const V3 &D, V3 &Po, V3 &Do)
{
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    Po = mk(object_row(r0, P, true), object_row(r1, P, true), object_row(r2, P, true));
    Do = mk(object_row(r0, D, false), object_row(r1, D, false), object_row(r2, D, false));
}

// the member scene of instance `inst`: its record's fourth row holds the scene slot
__device__ __forceinline__ const SceneView &leaf_view(const float4 *records, const SceneView *views, int inst)
{
    return views[__float_as_uint(records[4u * (uint32_t)inst + 3u].x)];
}

// the direction signs (bit c: D[c] >= 0) of the first lane of `walking`, a non-zero ballot: wave-uniform.  The ray kernels
// take a branch's lower child first when bit (link >> 29), its split axis, is set: near children first (the speed only)
__device__ __forceinline__ uint32_t first_lane_signs(const V3 &D, unsigned long long walking)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)((D.x >= 0.0f ? 1u : 0u) | (D.y >= 0.0f ? 2u : 0u) | (D.z >= 0.0f ? 4u : 0u)),
                                               (int)__builtin_ctzll(walking));
}

// The wave's walk of the top level from the root, called by the whole wave when any of its lanes walks; `top` is the wave's
// kTopStack words of LDS.  enters(node, a, b) is this lane's predicate on a node's two float4 (the caller keeps "the root is
// not tested" in it: a set of one instance culls nothing, so its walks are the plain query's).  At a branch that some lane
// enters, lower_first(link, left, entering) must be wave-uniform: the other child waits on the stack (every lane writes the
// same word; readfirstlane hands it back in an SGPR).  At such a leaf at_leaf(inst, enters) runs on every lane: the node
// index is wave-uniform by induction, so inst is, and what the caller fetches by it arrives by scalar loads.
template <class Enters, class LowerFirst, class AtLeaf>
__device__ __forceinline__ void walk_top_level(const TopNode *__restrict__ nodes, uint32_t *top, Enters &&enters_node,
                                               LowerFirst &&lower_first, AtLeaf &&at_leaf)
{
    uint32_t node = 0;
    int sp = 0;
    for (;;) {
        const float4 a = reinterpret_cast<const float4 *>(nodes)[2u * node];
        const float4 b = reinterpret_cast<const float4 *>(nodes)[2u * node + 1u];
        const bool enters = enters_node(node, a, b);
        const unsigned long long entering = __builtin_amdgcn_ballot_w64(enters);
        if (entering) {
            const uint32_t link = __float_as_uint(b.w);
            if (!(link & kLeafBit)) {
                const uint32_t left = link & 0x1fffffffu;
                const bool low_first = lower_first(link, left, entering);
                top[sp++] = low_first ? left + 1u : left;   // the other child waits (every lane writes the same word)
                node = low_first ? left : left + 1u;
                continue;
            }
            at_leaf((int)(link & ~kLeafBit), enters);
        }
        if (sp == 0)
            break;
        node = (uint32_t)__builtin_amdgcn_readfirstlane((int)top[--sp]);
    }
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

// Not in the header: for libshray_instance_point.so, libshray_instance_near.so and libshray_instance_overlap.so.  The set's current object_to_world floats on its device, float
// [count][12], the very floats it was created or last updated with, for a launch enqueued on `hip_stream` after this call.
// After a host update (and on first use) the upload is staged on that stream; after a device update the copy is the one
// that update's commit wrote, in stream order.  Host-only; makes the set's device current and waits for nothing.
extern "C" int shrayi_instance_set_forward_maps(shray_instance_set *set, void *hip_stream, const float **d_maps);

// Not in the header: for libshray_instance_intersect.so, whose instance form checks a range of triangles against its
// instance's scene before any launch.  The member scene of instance `instance`, as the set was created.  Host-only; reads
// nothing back, waits for nothing and touches no device.
extern "C" int shrayi_instance_set_member_scene(const shray_instance_set *set, int32_t instance, shray_scene **scene);
