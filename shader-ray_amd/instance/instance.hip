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
#include <numeric>
#include <vector>

#include "error_internal.h"
#include "kernel_stack_common.h"
#include "query_common.h"
#include "scene_access_internal.h"
#include "shader_ray_instance.h"

using namespace shray;

namespace {

constexpr int kTopStack = 32;              // per-wave top-level stack entries: the depth is at most ceil(log2 2^20) = 20
constexpr uint32_t kLeafBit = 0x80000000u; // a node link: leaf | instance, or axis << 29 | first child (the second follows it)
// The cull's margin factor: 128 ulps of 1 times the instance's condition ||A||inf * ||W||inf
constexpr double kMarginUlps = 128.0 / 16777216.0;

// A top-level node, two float4: (lo.xyz, margin factor k) and (hi.xyz, link bits).  A lane widens the box by k * |P|inf more.
struct TopNode {
    float lo[3], k;
    float hi[3];
    uint32_t link;
};
static_assert(sizeof(TopNode) == 32, "two float4");

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

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0; }

// the float nearest x on its side: rounds a box's low corner down and its high corner up
float round_down(double x)
{
    float f = (float)x;
    if ((double)f > x)
        f = std::nextafter(f, -INFINITY);
    return f;
}
float round_up(double x)
{
    float f = (float)x;
    if ((double)f < x)
        f = std::nextafter(f, INFINITY);
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

// W = the float rounding of the double inverse of object_to_world; false for a singular or non-finite map
bool invert(const float *m, float *out, double *condition)
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
            row_w += std::fabs((double)out[4 * r + col]);
        }
        out[4 * r + 3] = (float)wt;
        norm_a = std::max(norm_a, std::fabs((double)m[4 * r]) + std::fabs((double)m[4 * r + 1]) + std::fabs((double)m[4 * r + 2]));
        norm_w = std::max(norm_w, row_w);
    }
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(out[j]))
            return false;
    *condition = norm_a * norm_w;
    return std::isfinite(*condition);
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
        // the world box: the root box's 8 corners through object_to_world in double, widened by the margin
        const std::array<float, 6> &rb = root_box[found->second];
        BoxRef &b = boxes[i];
        for (int c = 0; c < 3; ++c) {
            b.lo[c] = INFINITY;
            b.hi[c] = -INFINITY;
        }
        for (int corner = 0; corner < 8; ++corner) {
            const double x[3] = {rb[(corner & 1) ? 3 : 0], rb[(corner & 2) ? 4 : 1], rb[(corner & 4) ? 5 : 2]};
            for (int r = 0; r < 3; ++r) {
                const double y = (double)m[4 * r] * x[0] + (double)m[4 * r + 1] * x[1] + (double)m[4 * r + 2] * x[2] + (double)m[4 * r + 3];
                b.lo[r] = std::min(b.lo[r], y);
                b.hi[r] = std::max(b.hi[r], y);
            }
        }
        // k * (|world box|inf + |b|inf); each lane adds k * |P|inf
        double box_reach = 0.0;
        for (int c = 0; c < 3; ++c)
            box_reach = std::max({box_reach, std::fabs(b.lo[c]), std::fabs(b.hi[c])});
        const double reach = box_reach + std::max({std::fabs((double)m[3]), std::fabs((double)m[7]), std::fabs((double)m[11])});
        b.k = kMarginUlps * condition;
        for (int c = 0; c < 3; ++c) {
            b.lo[c] -= b.k * reach;
            b.hi[c] += b.k * reach;
            b.centre[c] = 0.5 * (b.lo[c] + b.hi[c]);
        }
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

}   // namespace

struct shray_instance_set {
    std::vector<shray_scene *> scenes;
    Prepared host;
    SetDevice dev;
};

namespace {

int make_set(const std::vector<shray_scene *> &scenes, const float *object_to_world, Prepared &p, SetDevice &d)
{
    int rc = prepare(scenes, object_to_world, p);
    if (rc)
        return rc;
    return upload(p, d);
}

int set_device_of(const shray_instance_set *set)
{
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != set->host.device)
        HIP_TRY(hipSetDevice(set->host.device));
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
    rc = set_device_of(set);
    if (rc)
        return rc;
    const FrameView fr = query_frame(qp);
    const int levels = set->host.stack_levels;
    const size_t walk_lds = stack_lds_bytes(levels, kBatchBlock), lds = walk_lds + kTopStack * sizeof(uint32_t);
    const uint32_t top_offset = (uint32_t)(walk_lds / sizeof(uint32_t));
    const uint64_t blocks = ((uint64_t)count + kBatchBlock - 1) / kBatchBlock, per_launch = kRaysPerLaunch / kBatchBlock;
    QueryWork w{(const float4 *)d_rays, (float4 *)d_hits, (uint64_t)count, 0, d_counters};
    const SetDevice &d = set->dev;
    for (uint64_t first = 0; first < blocks; first += per_launch) {
        w.first_block = first;
        const dim3 grid((unsigned int)(blocks - first < per_launch ? blocks - first : per_launch));
        if (d_counters)
            hipLaunchKernelGGL((instance_kernel<true, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else if (qp->any_hit)
            hipLaunchKernelGGL((instance_kernel<false, true>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        else
            hipLaunchKernelGGL((instance_kernel<false, false>), grid, dim3(kBatchBlock), lds, stream, w, d.nodes, d.records, d.views,
                               d_instances, fr, levels, top_offset);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return fail(SHRAY_ERR_DEVICE, "instance query launch failed: %s", hipGetErrorString(e));
    }
    return SHRAY_OK;
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
    rc = set_device_of(set);
    if (rc)
        return rc;
    struct Buffers {
        void *rays = nullptr, *hits = nullptr, *instances = nullptr, *counters = nullptr;
        ~Buffers()
        {
            for (void *p : {rays, hits, instances, counters})
                if (p)
                    (void)hipFree(p);
        }
    } b;
    const size_t ray_bytes = (size_t)count * sizeof(shray_ray), hit_bytes = (size_t)count * sizeof(shray_hit);
    const size_t instance_bytes = (size_t)count * sizeof(int32_t);
    HIP_TRY(hipMalloc(&b.rays, ray_bytes));
    HIP_TRY(hipMalloc(&b.hits, hit_bytes));
    if (instances)
        HIP_TRY(hipMalloc(&b.instances, instance_bytes));
    if (out) {
        HIP_TRY(hipMalloc(&b.counters, sizeof(DeviceCounters) * kCounterShards));
        HIP_TRY(hipMemset(b.counters, 0, sizeof(DeviceCounters) * kCounterShards));
    }
    HIP_TRY(hipMemcpy(b.rays, rays, ray_bytes, hipMemcpyHostToDevice));
    rc = trace_device(set, qp, (const shray_ray *)b.rays, count, (shray_hit *)b.hits, (int32_t *)b.instances, nullptr,
                      (DeviceCounters *)b.counters);
    if (rc)
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (hits)
        HIP_TRY(hipMemcpy(hits, b.hits, hit_bytes, hipMemcpyDeviceToHost));
    if (instances)
        HIP_TRY(hipMemcpy(instances, b.instances, instance_bytes, hipMemcpyDeviceToHost));
    if (out) {
        DeviceCounters shards[kCounterShards];
        HIP_TRY(hipMemcpy(shards, b.counters, sizeof(shards), hipMemcpyDeviceToHost));
        for (const DeviceCounters &s : shards) {
            out->node_visits += s.node_visits;
            out->leaf_visits += s.leaf_visits;
            out->triangle_tests += s.triangle_tests;
            out->traversals += s.traversals;
            out->bad_hits += s.bad_hits;
        }
    }
    return SHRAY_OK;
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
    Prepared p;
    SetDevice d;
    const int rc = make_set(set->scenes, object_to_world ? object_to_world : set->host.object_to_world.data(), p, d);
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
    memcpy(out, set->host.world_to_object.data(), set->host.world_to_object.size() * sizeof(float));
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
