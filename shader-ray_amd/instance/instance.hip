// instance.hip -- include/shader_ray_instance.h: world-space rays through a set of placed scenes.
//
// The host builds a small top-level BVH over the instances' world boxes (object median splits, one instance per leaf).  The
// kernel walks it wave-uniformly, and at each leaf the lanes whose rays enter the leaf's box move their rays into the
// instance's object space and run the ray query's walk (query/query_common.h: the packed stack traversal in its convergent
// form), starting from the ray's best hit so far.  DESIGN.md section 10 argues the box margin and the uniformity of the views.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "client_internal.h"
#include "device_array_check.h"
#include "error_internal.h"
#include "kernel_stack_common.h"
#include "query_common.h"
#include "scene_access_internal.h"
#include "shader_ray_instance.h"
#include "top_level.h"

using namespace shray;

namespace {

// The cull's margin factor: 128 ulps of 1 times the instance's condition ||A||inf * ||W||inf
constexpr double kMarginUlps = 128.0 / 16777216.0;

// What a launch reads besides the rays: every pointer is __restrict__ in the kernel's arguments, so that the views come in
// by scalar loads (the traversal's inline asm takes their packed-array pointers as "s" operands)
struct SetDevice {
    TopNode *nodes = nullptr;     // [node_count], the root first
    float4 *records = nullptr;    // [count][4]: W's three rows, then (scene slot bits, 0, 0, 0)
    SceneView *views = nullptr;   // [distinct scenes]
};

void free_device(SetDevice &d)
{
    for (void *p : {(void *)d.nodes, (void *)d.records, (void *)d.views})
        if (p)
            (void)hipFree(p);
    d = SetDevice{};
}

// One-wave workgroups, as query_stack_kernel.  COUNT: the counting instance (closest-hit walks, the compiler's node stage).
template <bool COUNT, bool ANY_HIT>
__global__ void __launch_bounds__(kBatchBlock, COUNT ? SHRAY_MIN_WAVES_VIEW : SHRAY_MIN_WAVES_DEALT)
    instance_kernel(QueryWork w, const TopNode *__restrict__ nodes, const float4 *__restrict__ records,
                    const SceneView *__restrict__ views, int32_t *__restrict__ instances, FrameView fr, int stack_levels,
                    uint32_t top_offset)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    using Traversal = StackTraversal<kBatchBlock, true, false, false, false>;
    Traversal trav = make_traversal<true, kBatchBlock, false, false, false>(lds_stack, stack_levels);
    uint32_t *top = lds_stack + top_offset;   // the wave's top-level stack, after the traversal's LDS
    V3 P = mk(0, 0, 0), D = mk(0, 0, 1);
    float tmax = 0.0f;
    uint64_t index = 0;
    const bool live = query_ray<8>(fr, w, w.first_block + blockIdx.x, P, D, tmax, index);
    const bool traced = live && tmax > 0.0f;   // (false for NaN)
    Hit best{traced ? start_bound(tmax) : kFar, -1.0f, 0.0f, 0.0f};
    int best_instance = -1;
    bool active = traced;   // the ray walks on
    RayCounters rc = {0, 0, 0, 0, 0, 0, 0};
    const float pmax = fmaxf(fabsf(P.x), fmaxf(fabsf(P.y), fabsf(P.z)));
    const unsigned long long first = wave_ballot(active);
    if (first) {
        // near children first by the first live lane's direction signs (the walk's order affects its speed only)
        const uint32_t signs = (uint32_t)__builtin_amdgcn_readlane((int)((D.x >= 0.0f ? 1u : 0u) | (D.y >= 0.0f ? 2u : 0u) |
                                                                          (D.z >= 0.0f ? 4u : 0u)),
                                                                    (int)__builtin_ctzll(first));
        uint32_t node = 0;
        int sp = 0;
        for (;;) {
            const float4 a = reinterpret_cast<const float4 *>(nodes)[2u * node];
            const float4 b = reinterpret_cast<const float4 *>(nodes)[2u * node + 1u];
            // the root is not tested: a set of one instance culls nothing, so its walks are the plain query's
            const bool enters = active && (node == 0u || enters_box(a, b, P, D, a.w * pmax, best.t));
            if (wave_ballot(enters)) {
                const uint32_t link = __float_as_uint(b.w);
                if (!(link & kLeafBit)) {
                    const uint32_t left = link & 0x1fffffffu;
                    const bool low_first = (signs >> (link >> 29)) & 1u;
                    top[sp++] = low_first ? left + 1u : left;   // the far child waits (every lane writes the same word)
                    node = low_first ? left : left + 1u;
                    continue;
                }
                const int inst = (int)(link & ~kLeafBit);
                const float4 *rec = records + 4u * (uint32_t)inst;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                const SceneView &sc = views[__float_as_uint(rec[3].x)];
                const V3 Po = mk(object_row(r0, P, true), object_row(r1, P, true), object_row(r2, P, true));
                const V3 Do = mk(object_row(r0, D, false), object_row(r1, D, false), object_row(r2, D, false));
                // a lower instance wins a tie at the best t: its walk may accept t == best.t
                float start = best.t;
                if (best_instance > inst)
                    start = fminf(nextafterf(best.t, INFINITY), kRangeMax);
                Hit h{start, -1.0f, 0.0f, 0.0f};
                trav.template closest<COUNT, ANY_HIT && !COUNT>(sc, fr, enters, Po, Do, h, rc, start);
                if (enters) {
                    if (h.t == -1.0f) {          // the iteration cap: the ray ends
                        best = h;
                        best_instance = -1;
                        active = false;
                    } else if (h.which >= 0.0f && h.t < start) {
                        best = h;
                        best_instance = inst;
                        if (ANY_HIT && !COUNT)
                            active = false;
                    }
                }
            }
            if (sp == 0)
                break;
            node = (uint32_t)__builtin_amdgcn_readfirstlane((int)top[--sp]);
        }
    }
    if (live) {
        w.hits[index] = hit_record(best, traced, tmax);
        if (instances)
            instances[index] = best_instance;
    }
    if (COUNT) {
        if (traced && best.t == -1.0f)
            rc.bad_hits++;
        add_counters(rc, w.counters);
    }
}

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

// the top level over boxes[ids[first .. first + n)], node `at` (its children are allocated together)
void build_top(std::vector<TopNode> &nodes, std::vector<BoxRef> &boxes, std::vector<int32_t> &ids, size_t first, size_t n, size_t at)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double k = 0.0;
    for (size_t j = first; j < first + n; ++j) {
        const BoxRef &b = boxes[ids[j]];
        for (int c = 0; c < 3; ++c) {
            lo[c] = std::min(lo[c], b.lo[c]);
            hi[c] = std::max(hi[c], b.hi[c]);
            clo[c] = std::min(clo[c], b.centre[c]);
            chi[c] = std::max(chi[c], b.centre[c]);
        }
        k = std::max(k, b.k);
    }
    TopNode node;
    for (int c = 0; c < 3; ++c) {
        node.lo[c] = round_down(lo[c]);
        node.hi[c] = round_up(hi[c]);
    }
    node.k = round_up(k);
    if (n == 1) {
        node.link = kLeafBit | (uint32_t)ids[first];
        nodes[at] = node;
        return;
    }
    int axis = 0;
    for (int c = 1; c < 3; ++c)
        if (chi[c] - clo[c] > chi[axis] - clo[axis])
            axis = c;
    const size_t half = n / 2;
    std::nth_element(ids.begin() + first, ids.begin() + first + half, ids.begin() + first + n, [&](int32_t x, int32_t y) {
        const double cx = boxes[x].centre[axis], cy = boxes[y].centre[axis];
        return cx < cy || (cx == cy && x < y);
    });
    const size_t left = nodes.size();
    nodes.resize(left + 2);
    node.link = (uint32_t)axis << 29 | (uint32_t)left;
    nodes[at] = node;
    build_top(nodes, boxes, ids, first, half, left);
    build_top(nodes, boxes, ids, first + half, n - half, left + 1);
}

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

int prepare(const std::vector<shray_scene *> &scenes, const float *object_to_world, Prepared &p)
{
    const size_t n = scenes.size();
    p.object_to_world.assign(object_to_world, object_to_world + 12 * n);
    p.world_to_object.assign(12 * n, 0.0f);
    std::map<const shray_scene *, uint32_t> slot;
    std::vector<std::array<float, 6>> root_box;
    std::vector<BoxRef> boxes(n);
    p.records.assign(4 * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t i = 0; i < n; ++i) {
        const float *m = &p.object_to_world[12 * i];
        double condition = 0.0;
        if (!invert(m, &p.world_to_object[12 * i], &condition))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: the transform is non-finite or singular, or its inverse is not finite", i);
        auto found = slot.find(scenes[i]);
        if (found == slot.end()) {
            ShrayQueryScene q;
            if (!scenes[i])
                return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: the scene is NULL", i);
            const int rc = shrayi_scene_query_view(scenes[i], &q);
            if (rc)
                return rc;
            if (!q.packed_ok)
                return fail(SHRAY_ERR_BAD_TREE, "instance %zu: the scene has no packed tree (instances walk the packed stack traversal)", i);
            if (p.device < 0) {
                p.device = q.device;
                HIP_TRY(hipSetDevice(p.device));
                // work enqueued before this call on any stream (a refit of a member) completes before its root box is read
                HIP_TRY(hipDeviceSynchronize());
            } else if (q.device != p.device) {
                return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: its scene is on device %d, the set's on %d", i, q.device, p.device);
            }
            std::array<float, 6> box;
            const size_t root = 3u * (size_t)q.view.tree_root;
            HIP_TRY(hipMemcpy(box.data(), q.view.boxmin + root, 3 * sizeof(float), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(box.data() + 3, q.view.boxmax + root, 3 * sizeof(float), hipMemcpyDeviceToHost));
            found = slot.emplace(scenes[i], (uint32_t)p.views.size()).first;
            p.views.push_back(q.view);
            root_box.push_back(box);
            p.stack_levels = std::max(p.stack_levels, q.stack_levels);
        }
        place_box(m, root_box[found->second].data(), condition, boxes[i]);
        const float *wrow = &p.world_to_object[12 * i];
        for (int r = 0; r < 3; ++r)
            p.records[4 * i + r] = make_float4(wrow[4 * r], wrow[4 * r + 1], wrow[4 * r + 2], wrow[4 * r + 3]);
        uint32_t s = found->second;
        float sbits;
        memcpy(&sbits, &s, sizeof(s));
        p.records[4 * i + 3].x = sbits;
    }
    std::vector<int32_t> ids(n);
    std::iota(ids.begin(), ids.end(), 0);
    p.nodes.assign(1, TopNode{});
    build_top(p.nodes, boxes, ids, 0, n, 0);
    return SHRAY_OK;
}

int upload(const Prepared &p, SetDevice &d)
{
    struct Guard {
        SetDevice &d;
        bool keep = false;
        ~Guard() { if (!keep) free_device(d); }
    } guard{d};
    HIP_TRY(hipMalloc(&d.nodes, p.nodes.size() * sizeof(TopNode)));
    HIP_TRY(hipMalloc(&d.records, p.records.size() * sizeof(float4)));
    HIP_TRY(hipMalloc(&d.views, p.views.size() * sizeof(SceneView)));
    HIP_TRY(hipMemcpy(d.nodes, p.nodes.data(), p.nodes.size() * sizeof(TopNode), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.records, p.records.data(), p.records.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.views, p.views.data(), p.views.size() * sizeof(SceneView), hipMemcpyHostToDevice));
    guard.keep = true;
    return SHRAY_OK;
}

// ---- The device update (shray_instance_set_update_device) --------------------------------------------------------------------
//
// The host update's set, built on the set's device and stream-ordered.  One pass per instance runs
// invert and place_box, the host's own functions, and sets the refusal word; the ids are then sorted once per axis by
// (centre[axis], id), and the top level is built level by level from the three sorted lists: a segment's centroid extent on
// axis c is its last minus its first entry in list c, its left child takes the first count / 2 entries of the chosen axis's
// list, and the other two lists are partitioned stably by that flag, so every list stays in (key, id) order within each
// segment and each split is the set std::nth_element leaves on either side of the median.  Node positions are the host's
// pre-order allocation, a function of the counts alone (segment_at).  Boxes are folded bottom-up in float: the outward
// roundings are monotone, so the fold of the rounded leaf boxes is the rounding of the host's double fold.  Everything goes
// to scratch first; the last kernel copies it over the set's arrays unless an instance was refused.

constexpr int kUpdateBlock = 256;
constexpr int32_t kNoRefusal = 0x7f7f7f7f;   // the refusal word before the pass (a byte memset): above every instance index

// where sorted position p sits after `depth` levels of splits: the segment [first, first + count), its node, and (count >= 2)
// the position of its children's pair.  A node's left child holds count / 2 instances; its pair follows the parent's pair,
// and the right child's pair follows the left child's subtree of 2 * (count / 2) - 1 nodes (the host's pre-order allocation).
struct Segment {
    uint32_t first, count, node, pair;
};

__device__ __forceinline__ Segment segment_at(uint32_t p, uint32_t n, int depth)
{
    Segment g{0u, n, 0u, 1u};
    for (int d = 0; d < depth && g.count >= 2u; ++d) {
        const uint32_t half = g.count / 2u;
        if (p < g.first + half)
            g = Segment{g.first, half, g.pair, g.pair + 2u};
        else
            g = Segment{g.first + half, g.count - half, g.pair + 1u, g.pair + 2u * half};
    }
    return g;
}

// an unsigned key in the order of the doubles, -0 with +0 (c + 0.0 is +0 for either zero)
__device__ __forceinline__ uint64_t centre_key(double c)
{
    const uint64_t u = (uint64_t)__double_as_longlong(c + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ bool refused_already(const int32_t *refused) { return *refused != kNoRefusal; }

__global__ void __launch_bounds__(kUpdateBlock) iu_iota(uint32_t n, uint32_t *ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        ids[i] = i;
}

// one thread per instance: W, the leaf node, the centre and its keys; a refused transform lowers the refusal word
__global__ void __launch_bounds__(kUpdateBlock) iu_instances(uint32_t n, const float *__restrict__ object_to_world,
                                                             const float4 *__restrict__ live_records, const SceneView *__restrict__ views,
                                                             float4 *__restrict__ records, TopNode *__restrict__ leaves,
                                                             double *__restrict__ centres, uint64_t *__restrict__ keys, int32_t *refused)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float m[12], w[12];
    for (int j = 0; j < 12; ++j)
        m[j] = object_to_world[12 * (size_t)i + j];
    double condition = 0.0;
    if (!invert(m, w, &condition)) {
        atomicMin(refused, (int32_t)i);
        return;
    }
    const uint32_t slot = __float_as_uint(live_records[4 * (size_t)i + 3].x);   // (a set's scene slots never change)
    const SceneView &v = views[slot];
    const size_t root = 3u * (size_t)v.tree_root;
    const float rb[6] = {v.boxmin[root], v.boxmin[root + 1], v.boxmin[root + 2], v.boxmax[root], v.boxmax[root + 1], v.boxmax[root + 2]};
    BoxRef b;
    place_box(m, rb, condition, b);
    for (int r = 0; r < 3; ++r)
        records[4 * (size_t)i + r] = make_float4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    records[4 * (size_t)i + 3] = make_float4(__uint_as_float(slot), 0.0f, 0.0f, 0.0f);
    TopNode leaf;
    for (int c = 0; c < 3; ++c) {
        leaf.lo[c] = round_down(b.lo[c]);
        leaf.hi[c] = round_up(b.hi[c]);
        centres[(size_t)c * n + i] = b.centre[c];
        keys[(size_t)c * n + i] = centre_key(b.centre[c]);
    }
    leaf.k = round_up(b.k);
    leaf.link = kLeafBit | i;
    leaves[i] = leaf;
}

// level `depth`, one thread per sorted position: the split axis of the position's segment (the host's: the longest centroid
// extent, the lowest axis on a tie), its left-half flag by instance, and the node's link
__global__ void __launch_bounds__(kUpdateBlock) iu_split(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                         const double *__restrict__ centres, uint32_t *__restrict__ left_of,
                                                         TopNode *__restrict__ nodes, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    if (g.count < 2u)
        return;
    const uint32_t last = g.first + g.count - 1u;
    double extent[3];
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)c * n;
        extent[c] = centres[at + lists[at + last]] - centres[at + lists[at + g.first]];
    }
    int axis = 0;
    for (int c = 1; c < 3; ++c)
        if (extent[c] > extent[axis])
            axis = c;
    left_of[lists[(size_t)axis * n + p]] = p - g.first < g.count / 2u ? 1u : 0u;
    if (p == g.first)
        nodes[g.node].link = (uint32_t)axis << 29 | g.pair;
}

// every list's left-half flags by position (0 in segments that no longer split)
__global__ void __launch_bounds__(kUpdateBlock) iu_flags(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                         const uint32_t *__restrict__ left_of, uint32_t *__restrict__ flags,
                                                         const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const bool splits = segment_at(p, n, depth).count >= 2u;
    for (int c = 0; c < 3; ++c)
        flags[(size_t)c * n + p] = splits ? left_of[lists[(size_t)c * n + p]] : 0u;
}

// the stable partition of every list within each splitting segment: the left half first, each half in its old order
__global__ void __launch_bounds__(kUpdateBlock) iu_scatter(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                           const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offsets,
                                                           uint32_t *__restrict__ out, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)c * n;
        const uint32_t id = lists[at + p];
        if (g.count < 2u) {
            out[at + p] = id;
            continue;
        }
        const uint32_t before = offsets[at + p] - offsets[at + g.first];   // left entries in [first, p)
        out[at + (flags[at + p] ? g.first + before : g.first + g.count / 2u + (p - g.first - before))] = id;
    }
}

// after the last level every segment is one instance: its leaf node
__global__ void __launch_bounds__(kUpdateBlock) iu_leaves(uint32_t n, int depth, const uint32_t *__restrict__ lists,
                                                          const TopNode *__restrict__ leaves, TopNode *__restrict__ nodes,
                                                          const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    nodes[segment_at(p, n, depth).node] = leaves[lists[p]];
}

// level `depth`'s branches from their children's boxes (min / max are exact; the link was written by iu_split)
__global__ void __launch_bounds__(kUpdateBlock) iu_fold(uint32_t n, int depth, TopNode *nodes, const int32_t *refused)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || refused_already(refused))
        return;
    const Segment g = segment_at(p, n, depth);
    if (g.count < 2u || p != g.first)
        return;
    const TopNode a = nodes[g.pair], b = nodes[g.pair + 1u];
    TopNode t;
    for (int c = 0; c < 3; ++c) {
        t.lo[c] = (b.lo[c] < a.lo[c]) ? b.lo[c] : a.lo[c];
        t.hi[c] = (a.hi[c] < b.hi[c]) ? b.hi[c] : a.hi[c];
    }
    t.k = (a.k < b.k) ? b.k : a.k;
    t.link = nodes[g.node].link;
    nodes[g.node] = t;
}

// the scratch over the set's arrays, or nothing when an instance was refused; the outcome into the status word
__global__ void __launch_bounds__(kUpdateBlock) iu_commit(uint32_t n, const TopNode *__restrict__ new_nodes,
                                                          const float4 *__restrict__ new_records, const float *__restrict__ new_transforms,
                                                          const uint32_t *__restrict__ new_views, uint32_t view_words, TopNode *__restrict__ nodes,
                                                          float4 *__restrict__ records, float *__restrict__ transforms,
                                                          uint32_t *__restrict__ views, const int32_t *refused, int32_t *status)
{
    const int32_t r = *refused;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (first == 0)
        *status = r == kNoRefusal ? -1 : r;
    if (r != kNoRefusal)
        return;
    for (size_t k = first; k < 2 * (size_t)n - 1; k += stride)
        nodes[k] = new_nodes[k];
    for (size_t k = first; k < 4 * (size_t)n; k += stride)
        records[k] = new_records[k];
    if (new_transforms)
        for (size_t k = first; k < 12 * (size_t)n; k += stride)
            transforms[k] = new_transforms[k];
    for (size_t k = first; k < view_words; k += stride)
        views[k] = new_views[k];
}

// pinned host memory a copy reads from, free again once `copied` has completed
struct Staging {
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
};

// waits for every copy of `staging` and frees its pinned memory
void release(std::vector<Staging> &staging)
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
// it last uploaded.
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

}   // namespace

struct shray_instance_set {
    std::vector<shray_scene *> scenes;
    std::vector<shray_scene *> distinct;    // the member scenes by scene slot (prepare's: first appearance)
    Prepared host;
    SetDevice dev;
    std::unique_ptr<DeviceUpdate> update;   // the device update's state, once one was made
    std::unique_ptr<ForwardMaps> maps;      // the device copy of object_to_world, once something asked for it
    bool host_stale = false;                // host.object_to_world / world_to_object may be behind a device update
};

namespace {

int make_set(const std::vector<shray_scene *> &scenes, const float *object_to_world, Prepared &p, SetDevice &d)
{
    int rc = prepare(scenes, object_to_world, p);
    if (rc)
        return rc;
    return upload(p, d);
}

// ---- the device update's host side -------------------------------------------------------------------------------------------

unsigned int blocks_of(size_t items) { return (unsigned int)((items + kUpdateBlock - 1) / kUpdateBlock); }

// the scratch of the device update, made once per set on its device; the ids are written on `stream`
int make_update(shray_instance_set *set, hipStream_t stream, std::unique_ptr<DeviceUpdate> &out)
{
    auto u = std::make_unique<DeviceUpdate>();
    const uint32_t n = (uint32_t)set->scenes.size();
    u->n = n;
    while ((1u << u->depth) < n)
        u->depth++;
    for (shray_scene *s : set->scenes)
        if (std::find(u->distinct.begin(), u->distinct.end(), s) == u->distinct.end())
            u->distinct.push_back(s);
    const size_t m = 3 * (size_t)n;
    HIP_TRY(u->words.alloc(2 * sizeof(int32_t)));
    HIP_TRY(u->records.alloc(4 * (size_t)n * sizeof(float4)));
    HIP_TRY(u->leaves.alloc((size_t)n * sizeof(TopNode)));
    HIP_TRY(u->nodes.alloc((2 * (size_t)n - 1) * sizeof(TopNode)));
    HIP_TRY(u->centres.alloc(m * sizeof(double)));
    HIP_TRY(u->keys.alloc(m * sizeof(uint64_t)));
    HIP_TRY(u->sorted_keys.alloc(m * sizeof(uint64_t)));
    HIP_TRY(u->ids.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(u->lists[0].alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->lists[1].alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->left_of.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(u->flags.alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->offsets.alloc(m * sizeof(uint32_t)));
    HIP_TRY(u->views.alloc(u->distinct.size() * sizeof(SceneView)));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)n, 0, 64, stream));
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, m,
                                    rocprim::plus<uint32_t>(), stream));
    u->temp_bytes = std::max(sort_bytes, scan_bytes);
    HIP_TRY(u->temp.alloc(u->temp_bytes));
    HIP_TRY(hipEventCreateWithFlags(&u->finished, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(u->words.p, 0xff, 2 * sizeof(int32_t), stream));   // status -1: no update refused yet
    hipLaunchKernelGGL(iu_iota, dim3(blocks_of(n)), dim3(kUpdateBlock), 0, stream, n, u->ids.as<uint32_t>());
    if (const int rc = launched("instance update set-up"))
        return rc;
    out = std::move(u);
    return SHRAY_OK;
}

// `bytes` of host memory to device memory at `dst` on `stream`, through pinned memory that is reused once its copy is done
// (no host wait)
int stage(std::vector<Staging> &staging, hipStream_t stream, void *dst, const void *src, size_t bytes)
{
    Staging *s = nullptr;
    for (Staging &c : staging) {
        const hipError_t q = hipEventQuery(c.copied);
        if (q == hipSuccess && c.bytes >= bytes) {
            s = &c;
            break;
        }
        if (q != hipSuccess)
            (void)hipGetLastError();   // (hipErrorNotReady is an answer here, not an error for the launches after this)
    }
    if (!s) {
        Staging c;
        c.bytes = bytes;
        HIP_TRY(hipHostMalloc(&c.host, bytes, hipHostMallocDefault));
        const hipError_t e = hipEventCreateWithFlags(&c.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipHostFree(c.host);
            return fail(SHRAY_ERR_DEVICE, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        staging.push_back(c);
        s = &staging.back();
    }
    memcpy(s->host, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, s->host, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->copied, stream));
    return SHRAY_OK;
}

// The device copy of the set's object-to-world maps, current for work enqueued on `stream` after this call: made on first
// use (12 n floats, nothing else), uploaded from the host copy on `stream` when it is behind it, else `stream` waits for the
// last upload, which may have run on another stream.  No host wait.  (The set's device is current.)
int current_maps(shray_instance_set *set, hipStream_t stream)
{
    if (!set->maps) {
        auto m = std::make_unique<ForwardMaps>();
        HIP_TRY(m->transforms.alloc(12 * set->scenes.size() * sizeof(float)));
        HIP_TRY(hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming));
        set->maps = std::move(m);
    }
    ForwardMaps &m = *set->maps;
    if (m.stale) {
        const int rc = stage(m.staging, stream, m.transforms.p, set->host.object_to_world.data(), 12 * set->scenes.size() * sizeof(float));
        if (rc)
            return rc;
        HIP_TRY(hipEventRecord(m.uploaded, stream));
        m.recorded = true;
        m.stale = false;
    } else if (m.recorded) {
        HIP_TRY(hipStreamWaitEvent(stream, m.uploaded, 0));
    }
    return SHRAY_OK;
}

// the host copies of the transforms and W after a device update: waits for it and downloads them
int refresh_host(shray_instance_set *set)
{
    if (!set->host_stale)
        return SHRAY_OK;
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    const size_t n = set->scenes.size();
    std::vector<float4> records(4 * n);
    std::vector<float> transforms(12 * n);
    HIP_TRY(hipEventSynchronize(set->update->finished));
    HIP_TRY(hipMemcpy(records.data(), set->dev.records, records.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(transforms.data(), set->maps->transforms.p, transforms.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            const float4 &w = records[4 * i + r];
            float *out = &set->host.world_to_object[12 * i + 4 * r];
            out[0] = w.x;
            out[1] = w.y;
            out[2] = w.z;
            out[3] = w.w;
        }
    set->host.object_to_world = std::move(transforms);
    set->host.records = std::move(records);
    set->host_stale = false;
    return SHRAY_OK;
}

int update_device(shray_instance_set *set, const float *d_object_to_world, hipStream_t stream)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    const uint32_t n = (uint32_t)set->scenes.size();
    if (d_object_to_world) {
        if (!aligned(d_object_to_world, 4))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "object_to_world must be 4-byte aligned");
        rc = check_device_array(d_object_to_world, 12 * (size_t)n * sizeof(float), set->host.device, "object_to_world", "set");
        if (rc)
            return rc;
    }
    if (!set->update) {
        rc = make_update(set, stream, set->update);
        if (rc)
            return rc;
    }
    DeviceUpdate &u = *set->update;
    // the member views as they are now (a refit may have flipped exact_div_ok), uploaded when they changed
    std::vector<SceneView> views(u.distinct.size());
    for (size_t k = 0; k < views.size(); ++k) {
        ShrayQueryScene q;
        rc = shrayi_scene_query_view(u.distinct[k], &q);
        if (rc)
            return rc;
        views[k] = q.view;
    }
    const size_t view_bytes = views.size() * sizeof(SceneView);
    if (!u.views_staged || memcmp(views.data(), u.staged.data(), view_bytes) != 0) {
        rc = stage(u.staging, stream, u.views.p, views.data(), view_bytes);
        if (rc)
            return rc;
        u.staged = views;
        u.views_staged = true;
    }
    if ((rc = current_maps(set, stream)))
        return rc;
    const DeviceBuffer &transforms = set->maps->transforms;
    int32_t *refused = u.words.as<int32_t>();
    const size_t m = 3 * (size_t)n;
    const dim3 grid(blocks_of(n)), block(kUpdateBlock);
    HIP_TRY(hipMemsetAsync(refused, 0x7f, sizeof(int32_t), stream));   // kNoRefusal
    // 1. one pass per instance
    hipLaunchKernelGGL(iu_instances, grid, block, 0, stream, n, d_object_to_world ? d_object_to_world : transforms.as<const float>(),
                       (const float4 *)set->dev.records, u.views.as<const SceneView>(), u.records.as<float4>(), u.leaves.as<TopNode>(),
                       u.centres.as<double>(), u.keys.as<uint64_t>(), refused);
    if ((rc = launched("instance update")))
        return rc;
    // 2. the ids by (centre[c], id), once per axis
    uint32_t *lists = u.lists[0].as<uint32_t>(), *spare = u.lists[1].as<uint32_t>();
    for (int c = 0; c < 3; ++c) {
        size_t bytes = u.temp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(u.temp.p, bytes, u.keys.as<const uint64_t>() + (size_t)c * n, u.sorted_keys.as<uint64_t>() + (size_t)c * n,
                                          u.ids.as<const uint32_t>(), lists + (size_t)c * n, (size_t)n, 0, 64, stream));
    }
    // 3. the levels, top-down
    for (int d = 0; d < u.depth; ++d) {
        hipLaunchKernelGGL(iu_split, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.centres.as<const double>(),
                           u.left_of.as<uint32_t>(), u.nodes.as<TopNode>(), (const int32_t *)refused);
        hipLaunchKernelGGL(iu_flags, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.left_of.as<const uint32_t>(),
                           u.flags.as<uint32_t>(), (const int32_t *)refused);
        size_t bytes = u.temp_bytes;
        HIP_TRY(rocprim::exclusive_scan(u.temp.p, bytes, u.flags.as<const uint32_t>(), u.offsets.as<uint32_t>(), 0u, m,
                                        rocprim::plus<uint32_t>(), stream));
        hipLaunchKernelGGL(iu_scatter, grid, block, 0, stream, n, d, (const uint32_t *)lists, u.flags.as<const uint32_t>(),
                           u.offsets.as<const uint32_t>(), spare, (const int32_t *)refused);
        std::swap(lists, spare);
    }
    // 4. the leaves, then the boxes bottom-up
    hipLaunchKernelGGL(iu_leaves, grid, block, 0, stream, n, u.depth, (const uint32_t *)lists, u.leaves.as<const TopNode>(),
                       u.nodes.as<TopNode>(), (const int32_t *)refused);
    for (int d = u.depth - 1; d >= 0; --d)
        hipLaunchKernelGGL(iu_fold, grid, block, 0, stream, n, d, u.nodes.as<TopNode>(), (const int32_t *)refused);
    // 5. the commit
    const uint32_t view_words = (uint32_t)(view_bytes / sizeof(uint32_t));
    hipLaunchKernelGGL(iu_commit, dim3(std::min(blocks_of(12 * (size_t)n), 1024u)), block, 0, stream, n, u.nodes.as<const TopNode>(),
                       u.records.as<const float4>(), d_object_to_world, u.views.as<const uint32_t>(), view_words, set->dev.nodes,
                       set->dev.records, d_object_to_world ? transforms.as<float>() : nullptr, (uint32_t *)set->dev.views,
                       (const int32_t *)refused, refused + 1);
    if ((rc = launched("instance update")))
        return rc;
    HIP_TRY(hipEventRecord(u.finished, stream));
    u.enqueued = true;
    set->host_stale = true;
    return SHRAY_OK;
}

int trace_device(shray_instance_set *set, const shray_query_params *qp, const shray_ray *d_rays, int64_t count, shray_hit *d_hits,
                 int32_t *d_instances, hipStream_t stream, DeviceCounters *d_counters)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!set || !d_rays || !d_hits)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, rays or hits is NULL");
    if (!aligned(d_rays, 16) || !aligned(d_hits, 16) || !aligned(d_instances, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "ray and hit buffers must be 16-byte aligned, the instance buffer 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    rc = use_device(set->host.device);
    if (rc)
        return rc;
    const FrameView fr = query_frame(qp);
    const int levels = set->host.stack_levels;
    const size_t walk_lds = stack_lds_bytes(levels, kBatchBlock), lds = walk_lds + kTopStack * sizeof(uint32_t);
    const uint32_t top_offset = (uint32_t)(walk_lds / sizeof(uint32_t));
    const uint64_t blocks = ((uint64_t)count + kBatchBlock - 1) / kBatchBlock, per_launch = kRaysPerLaunch / kBatchBlock;
    QueryWork w{(const float4 *)d_rays, (float4 *)d_hits, (uint64_t)count, 0, d_counters};
    const SetDevice &d = set->dev;
    return for_each_launch(blocks, per_launch, [&](uint64_t first, dim3 grid) {
        w.first_block = first;
        if (d_counters)
            hipLaunchKernelGGL((instance_kernel<true, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else if (qp->any_hit)
            hipLaunchKernelGGL((instance_kernel<false, true>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else
            hipLaunchKernelGGL((instance_kernel<false, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        return launched("instance query");
    });
}

// the blocking forms: the rays to the device, the query on the null stream, the results (and tallies) back
int trace_host(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count, shray_hit *hits,
               int32_t *instances, shray_counters *out)
{
    int rc = check_params(qp);
    if (rc)
        return rc;
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative ray count %lld", (long long)count);
    if (!set || !rays)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or rays is NULL");
    if (out) {
        memset(out, 0, sizeof(*out));
        out->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    rc = use_device(set->host.device);
    if (rc)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{rays, n * sizeof(shray_ray)}}, {{hits, n * sizeof(shray_hit)}, {instances, instances ? n * sizeof(int32_t) : 0}}, out,
                        [&](DeviceBuffer *d_rays, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return trace_device(set, qp, d_rays->as<const shray_ray>(), count, d_out[0].as<shray_hit>(),
                                                d_out[1].as<int32_t>(), nullptr, shards);
                        });
}

}   // namespace

extern "C" {

int shray_instance_set_create(const shray_instance *instances, int32_t count, shray_instance_set **out)
{
    if (!instances || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "instances or out is NULL");
    *out = nullptr;
    if (count <= 0 || count > SHRAY_INSTANCE_MAX)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance count %d is outside [1, 2^20]", count);
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0)
        return fail(SHRAY_ERR_NO_DEVICE, "no HIP device is visible");
    std::vector<shray_scene *> scenes((size_t)count);
    std::vector<float> transforms(12 * (size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        scenes[i] = instances[i].scene;
        memcpy(&transforms[12 * (size_t)i], instances[i].object_to_world, 12 * sizeof(float));
    }
    shray_instance_set *set = new shray_instance_set;
    set->scenes = std::move(scenes);
    for (shray_scene *s : set->scenes)
        if (std::find(set->distinct.begin(), set->distinct.end(), s) == set->distinct.end())
            set->distinct.push_back(s);
    const int rc = make_set(set->scenes, transforms.data(), set->host, set->dev);
    if (rc) {
        delete set;
        return rc;
    }
    *out = set;
    return SHRAY_OK;
}

int shray_instance_set_update(shray_instance_set *set, const float *object_to_world)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    int rc = object_to_world ? SHRAY_OK : refresh_host(set);   // (the transforms of a device update)
    if (rc)
        return rc;
    Prepared p;
    SetDevice d;
    rc = make_set(set->scenes, object_to_world ? object_to_world : set->host.object_to_world.data(), p, d);
    if (rc)
        return rc;
    // queries in flight read the old arrays
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        free_device(d);
        return fail(SHRAY_ERR_DEVICE, "hipDeviceSynchronize failed: %s", hipGetErrorString(e));
    }
    free_device(set->dev);
    set->host = std::move(p);
    set->dev = d;
    set->host_stale = false;
    if (set->maps)
        set->maps->stale = true;
    return SHRAY_OK;
}

int shray_instance_set_update_device(shray_instance_set *set, const float *d_object_to_world, void *hip_stream)
{
    return update_device(set, d_object_to_world, (hipStream_t)hip_stream);
}

int shray_instance_set_update_status(shray_instance_set *set, int32_t *refused)
{
    if (!set || !refused)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or refused is NULL");
    *refused = -1;
    if (!set->update || !set->update->enqueued)
        return SHRAY_OK;
    const int rc = use_device(set->host.device);
    if (rc)
        return rc;
    HIP_TRY(hipEventSynchronize(set->update->finished));
    HIP_TRY(hipMemcpy(refused, set->update->words.as<int32_t>() + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

void shray_instance_set_destroy(shray_instance_set *set)
{
    if (!set)
        return;
    if (set->host.device >= 0 && hipSetDevice(set->host.device) == hipSuccess)
        free_device(set->dev);
    delete set;
}

int shray_instance_set_count(const shray_instance_set *set, int32_t *count)
{
    if (!set || !count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or count is NULL");
    *count = (int32_t)set->scenes.size();
    return SHRAY_OK;
}

int shray_instance_set_world_to_object(const shray_instance_set *set, float *out)
{
    if (!set || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or out is NULL");
    const int rc = refresh_host(const_cast<shray_instance_set *>(set));
    if (rc)
        return rc;
    memcpy(out, set->host.world_to_object.data(), set->host.world_to_object.size() * sizeof(float));
    return SHRAY_OK;
}

// For tests, not in the header: the set's top-level nodes (2 count - 1 of 32 bytes: lo.xyz, k, hi.xyz, link) and records
// (count * 4 float4: W's rows, then the scene slot) as the next query reads them, after any device update has finished.
// nodes and records may be NULL; *node_count, unless NULL, gets the node count.
int shrayi_instance_set_arrays(const shray_instance_set *set, void *nodes, void *records, int32_t *node_count)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    const size_t n = set->scenes.size();
    if (node_count)
        *node_count = (int32_t)(2 * n - 1);
    if (!nodes && !records)
        return SHRAY_OK;
    const int rc = use_device(set->host.device);
    if (rc)
        return rc;
    if (set->update && set->update->enqueued)
        HIP_TRY(hipEventSynchronize(set->update->finished));
    if (nodes)
        HIP_TRY(hipMemcpy(nodes, set->dev.nodes, (2 * n - 1) * sizeof(TopNode), hipMemcpyDeviceToHost));
    if (records)
        HIP_TRY(hipMemcpy(records, set->dev.records, 4 * n * sizeof(float4), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

// For libshray_instance_multihit.so, not in the header (top_level.h): the set's device arrays as the next launch reads them
// and its distinct member scenes.  Device pointers: nothing is copied, nothing waited for, no device touched.
int shrayi_instance_set_device_arrays(const shray_instance_set *set, ShrayInstanceSetDevice *out)
{
    if (!set || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or out is NULL");
    out->nodes = set->dev.nodes;
    out->records = set->dev.records;
    out->views = set->dev.views;
    out->scenes = set->distinct.data();
    out->count = (int32_t)set->scenes.size();
    out->scene_count = (int32_t)set->distinct.size();
    out->device = set->host.device;
    return SHRAY_OK;
}

// For libshray_instance_point.so, not in the header (top_level.h): the set's current object_to_world floats on its device,
// float [count][12], the very floats it was created or last updated with, for a launch enqueued on `hip_stream` after this
// call.  After a host update (and on first use) the upload is staged on that stream; after a device update the copy is the
// one that update's commit wrote, in stream order.  Host-only; makes the set's device current and waits for nothing.
int shrayi_instance_set_forward_maps(shray_instance_set *set, void *hip_stream, const float **d_maps)
{
    if (!set || !d_maps)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or d_maps is NULL");
    *d_maps = nullptr;
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    if ((rc = current_maps(set, (hipStream_t)hip_stream)))
        return rc;
    *d_maps = set->maps->transforms.as<const float>();
    return SHRAY_OK;
}

int shray_trace_instances_device(shray_instance_set *set, const shray_query_params *qp, const shray_ray *d_rays, int64_t count,
                                 shray_hit *d_hits, int32_t *d_instances, void *hip_stream)
{
    return trace_device(set, qp, d_rays, count, d_hits, d_instances, (hipStream_t)hip_stream, nullptr);
}

int shray_trace_instances(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                          shray_hit *hits, int32_t *instances)
{
    if (!hits && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "hits is NULL");
    return trace_host(set, qp, rays, count, hits, instances, nullptr);
}

int shray_trace_instances_counters(shray_instance_set *set, const shray_query_params *qp, const shray_ray *rays, int64_t count,
                                   shray_hit *hits, int32_t *instances, shray_counters *out)
{
    if (!out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return trace_host(set, qp, rays, count, hits, instances, out);
}

}   // extern "C"
