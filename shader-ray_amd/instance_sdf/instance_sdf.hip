// instance_sdf.hip -- include/shader_ray_instance_sdf.h: signed distances from world-space points to a set of placed scenes,
// the magnitude measured in world space, the sign decided in the nearest instance's object space.
//
// Stage 1 is libshray_instance_point.so's device form on the caller's stream: the world record and the instance of every
// point, into the caller's buffers or into stream-ordered scratch.  Nothing of it is compiled here.
// Stage 2 is this file's kernel, one lane per point in one-wave workgroups.  The lanes of a wave hold different instances, so
// the wave peels: while a lane is unsigned, the instance of the first such lane is made wave-uniform, its W rows, its scene
// slot, the member's SceneView and the member's sign data pointer arrive by scalar loads, and exactly the lanes that hold that
// instance map their point to object space, run point/point_walk.h's loop on the member's packed tree there, load the
// pseudonormal of the record's region and sign their value.  The sign data belongs to libshray_sdf.so, which hands out each
// member scene's pointer, current on the stream (shrayi_scene_sign_data).
// This is the first instanced client that uses other client libraries; it does so through their C entry points only and
// compiles none of their kernels, so their code objects do not change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "client_internal.h"
#include "closest_on_triangle.h"
#include "enter_set.h"
#include "packed_walk.h"
#include "shader_ray_instance_sdf.h"
#include "top_level.h"
#include "trace_common.h"

using namespace shray;

// libshray_sdf.so's, outside its header: a scene's sign data on its device, current for work enqueued on `hip_stream` after
// the call (derived there when stale).  Host-only; waits for nothing.
extern "C" int shrayi_scene_sign_data(shray_scene *scene, void *hip_stream, const float **d_sign);

namespace {

constexpr uint64_t kChunk = 1ull << 22;   // points per scratch chunk when the caller keeps no records or no instances
constexpr int kSlotsPerLaunch = 256;      // sign-data pointers one table launch carries in its arguments (2 KiB)

// the sign data of one triangle (SHRAY_SIGN_DATA_FLOATS): nhat, the vertex pseudonormals of corners a, b, c, the edge
// pseudonormals of AB, AC, BC
constexpr int kFaceAt = 0, kVertexAt = 3, kEdgeAt = 12;

struct SignSlots {
    const float *sign[kSlotsPerLaunch];
};

// The per-slot table of sign-data pointers reaches the device as a launch's arguments: stream-ordered, with no staging
// memory whose lifetime the host would have to watch.
__global__ void __launch_bounds__(kSlotsPerLaunch) store_sign_slots(const float **table, SignSlots slots, int n)
{
    if ((int)threadIdx.x < n)
        table[threadIdx.x] = slots.sign[threadIdx.x];
}

struct SignWork {
    const float4 *points;       // (p, max_dist2), world space
    const float4 *records;      // stage 1's: 2 per point
    const int32_t *instances;   // stage 1's: one per point, -1 on a miss
    float *out;                 // the signed values
    uint64_t count;
    uint64_t first;             // this launch's first point
    int32_t instance_count;     // the set's: an index outside it is signed as a miss's is, and selects nothing
    DeviceCounters *counters;
};

// One lane per point (file comment).  COUNT: the counting instance.  The set's records, the views and the table are
// __restrict__ so that what the peeled instance selects comes in by scalar loads.
template <bool COUNT>
__global__ void __launch_bounds__(kBlock) instance_sign_kernel(SignWork w, const float4 *__restrict__ set_records,
                                                               const SceneView *__restrict__ views,
                                                               const float *const *__restrict__ sign_of_slot)
{
    extern __shared__ __attribute__((aligned(16))) uint2 stack[];
    uint2 *column = stack + threadIdx.x;   // (node name, bound), level-major
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 in = make_float4(0.0f, 0.0f, 0.0f, -1.0f), r0 = in, r1 = make_float4(0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS), 0.0f);
    int inst = -1;
    if (live) {
        in = w.points[index];
        r0 = w.records[2 * index];
        r1 = w.records[2 * index + 1];
        inst = w.instances[index];
    }
    const int world_tri = __float_as_int(r1.z);
    bool unsigned_yet = live && world_tri >= 0 && inst >= 0 && inst < w.instance_count;   // a hit: its value's sign is still to be decided
    // a hit's value until its sign says otherwise; NaN on a miss
    float value = unsigned_yet ? sqrtf(r0.w) : __uint_as_float(0x7fc00000u);
    unsigned int nodes = 0, leaves = 0, tests = 0, walks = 0;

    unsigned long long pending = __builtin_amdgcn_ballot_w64(unsigned_yet);
    while (pending) {
        // the instance of the first unsigned lane, wave-uniform; what it selects arrives by scalar loads
        const int cur_inst = __builtin_amdgcn_readlane(inst, (int)__builtin_ctzll(pending));
        const float4 *rec = set_records + 4u * (uint32_t)cur_inst;
        const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
        const uint32_t slot = __float_as_uint(rec[3].x);
        const SceneView &sc = views[slot];
        const float *sign = sign_of_slot[slot];
        if (unsigned_yet && inst == cur_inst) {
            unsigned_yet = false;
            walks++;
            const V3 pw = mk(in.x, in.y, in.z);
            const float p[3] = {object_row(w0, pw, true), object_row(w1, pw, true), object_row(w2, pw, true)};
            // A non-finite p_o is a miss of the object-space query: sigma is NaN and the value stays positive.
            if (__builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2])) {
                // The seed.  The walk below must return the record of the +inf walk: the least (dist2, triangle) over all
                // triangles, D* at t*.  The world record's own triangle t is one of them, so its dist2 at p_o, d_t, is not
                // below D*; the condition dist2 <= max_dist2 is inclusive, so with max_dist2 = d_t every triangle at D*
                // still qualifies, t* among them, and the walk skips a node only when its bound is strictly above the best
                // so far.  The record is therefore the +inf one bit for bit, found among no more nodes than that walk visits
                // (DESIGN section 26 measures how many fewer).  A NaN d_t orders nothing, and a triangle index the member does
                // not have is not read: both start from +inf.
                float best = __uint_as_float(0x7f800000u);
                if ((uint32_t)world_tri < sc.triangle_count) {
                    const float d_t = closest_on_triangle(p, sc.positions + 9ull * (uint32_t)world_tri).dist2;
                    best = d_t == d_t ? d_t : best;
                }
                int best_tri = SHRAY_HIT_MISS;
                Closest found;
                found.q[0] = p[0], found.q[1] = p[1], found.q[2] = p[2];
                found.u = 0.0f, found.v = 0.0f, found.region = SHRAY_REGION_NONE;

                // point/point_walk.h's loop, on the member's packed tree in object space
                const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
                Record cur = load_record(copy, sc.packed_root);
                nodes++;
                int sp = 0;
                bool go = !(box_bound(p, cur.box.lo, cur.box.hi) > best);
                while (go) {
                    if (cur.b & kLeafFlag) {
                        leaves++;
                        const uint32_t first = cur.a, n = cur.b & ~kLeafFlag;
                        for (uint32_t t = first; t < first + n; t++) {
                            tests++;
                            const Closest c = closest_on_triangle(p, sc.positions + 9ull * t);
                            const bool better = best_tri < 0 ? c.dist2 <= best : (c.dist2 < best || (c.dist2 == best && (int)t < best_tri));
                            if (better) {
                                best = c.dist2;
                                best_tri = (int)t;
                                found = c;
                            }
                        }
                    } else {
                        const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
                        const Record c0 = load_record(copy, n0), c1 = load_record(copy, n1);
                        const float lb0 = box_bound(p, c0.box.lo, c0.box.hi), lb1 = box_bound(p, c1.box.lo, c1.box.hi);
                        nodes += 2;
                        const bool second = lb1 < lb0;   // the nearer child first
                        const float near_lb = second ? lb1 : lb0, far_lb = second ? lb0 : lb1;
                        if (!(near_lb > best)) {
                            if (!(far_lb > best)) {
                                column[(size_t)sp * kBlock] = make_uint2(second ? n0 : n1, __float_as_uint(far_lb));
                                sp++;
                            }
                            cur = second ? c1 : c0;
                            continue;
                        }
                        // near_lb <= far_lb: both children are out of reach
                    }
                    // pop the next node still in reach; the stack holds at most one entry per level of the current path
                    go = false;
                    while (sp > 0) {
                        sp--;
                        const uint2 e = column[(size_t)sp * kBlock];
                        if (!(__uint_as_float(e.y) > best)) {
                            cur = load_record(copy, e.x);
                            go = true;
                            break;
                        }
                    }
                }
                if (best_tri >= 0) {
                    const int region = found.region;
                    const int at = region == SHRAY_REGION_FACE ? kFaceAt
                                                               : region <= SHRAY_REGION_C ? kVertexAt + 3 * region : kEdgeAt + 3 * (region - SHRAY_REGION_AB);
                    const float *nrm = sign + (size_t)SHRAY_SIGN_DATA_FLOATS * (uint32_t)best_tri + at;
                    const float sigma = dot3(mk(p[0] - found.q[0], p[1] - found.q[1], p[2] - found.q[2]), mk(nrm[0], nrm[1], nrm[2]));
                    // (shray_signed_distance's own value is negative only off the surface: the object dist2 above 0)
                    if (sigma < 0.0f && best > 0.0f && r0.w > 0.0f)
                        value = -value;
                }
            }
        }
        pending = __builtin_amdgcn_ballot_w64(unsigned_yet);
    }
    if (live)
        w.out[index] = value;
    if (COUNT) {   // (every lane of the wave is here)
        const unsigned long long s0 = wave_sum(nodes), s1 = wave_sum(leaves), s2 = wave_sum(tests), s3 = wave_sum(walks);
        if (threadIdx.x == 0) {
            DeviceCounters *c = &w.counters[blockIdx.x % kCounterShards];
            atomicAdd(&c->node_visits, s0);
            atomicAdd(&c->leaf_visits, s1);
            atomicAdd(&c->triangle_tests, s2);
            atomicAdd(&c->traversals, s3);
        }
    }
}

// every distinct member scene's sign data current on `stream`, and the table of their pointers, by scene slot, written to
// `table` in stream order
int stage_sign_slots(const ShrayInstanceSetDevice &d, const float **table, hipStream_t stream)
{
    for (int32_t base = 0; base < d.scene_count; base += kSlotsPerLaunch) {
        const int n = std::min<int32_t>(kSlotsPerLaunch, d.scene_count - base);
        SignSlots slots;
        memset(&slots, 0, sizeof(slots));
        for (int k = 0; k < n; k++)
            if (const int rc = shrayi_scene_sign_data(d.scenes[base + k], stream, &slots.sign[k]))
                return rc;
        hipLaunchKernelGGL(store_sign_slots, dim3(1), dim3(kSlotsPerLaunch), 0, stream, table + base, slots, n);
        if (const int rc = launched("instanced signed-distance sign table"))
            return rc;
    }
    return SHRAY_OK;
}

int signed_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float *d_signed, shray_closest *d_closest,
                  int32_t *d_instances, hipStream_t stream, DeviceCounters *d_counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!set || !d_points || !d_signed)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, points or signed is NULL");
    if (!aligned(d_points, 16) || !aligned(d_closest, 16) || !aligned(d_signed, 4) || !aligned(d_instances, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT,
                    "point and record buffers must be 16-byte aligned, the signed values and the instance buffer 4-byte aligned");
    if (count == 0)
        return SHRAY_OK;
    ShrayInstanceSetDevice d;
    int height = 0;
    int rc = enter_set(set, &d, &height);   // (a member tree that is too high is refused here, before any launch)
    if (rc)
        return rc;
    const uint64_t n = (uint64_t)count;
    // the walk, then the sign, a chunk at a time; what the caller does not keep of stage 1 lives in stream-ordered scratch of
    // at most kChunk points
    const uint64_t chunk = d_closest && d_instances ? n : std::min(n, kChunk);
    const size_t table_bytes = (size_t)d.scene_count * sizeof(const float *);
    const size_t records_at = (table_bytes + 255) & ~(size_t)255;
    const size_t instances_at = records_at + (d_closest ? 0 : chunk * sizeof(shray_closest));
    const size_t total = instances_at + (d_instances ? 0 : chunk * sizeof(int32_t));
    char *scratch = nullptr;
    HIP_TRY(hipMallocAsync((void **)&scratch, total, stream));
    const float **table = reinterpret_cast<const float **>(scratch);
    rc = stage_sign_slots(d, table, stream);
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint2);   // a lane's column: one entry per level of the tallest member
    for (uint64_t first = 0; first < n && !rc; first += chunk) {
        const uint64_t m = std::min(chunk, n - first);
        shray_closest *records = d_closest ? d_closest + first : reinterpret_cast<shray_closest *>(scratch + records_at);
        int32_t *instances = d_instances ? d_instances + first : reinterpret_cast<int32_t *>(scratch + instances_at);
        rc = shray_closest_points_instances_device(set, d_points + first, (int64_t)m, records, instances, stream);
        if (rc)
            break;
        SignWork w{(const float4 *)(d_points + first), (const float4 *)records, instances, d_signed + first, m, 0, d.count, d_counters};
        rc = for_each_launch((m + kBlock - 1) / kBlock, kPointsPerLaunch / kBlock, [&](uint64_t first_block, dim3 grid) {
            w.first = first_block * kBlock;
            if (d_counters)
                hipLaunchKernelGGL(instance_sign_kernel<true>, grid, dim3(kBlock), lds, stream, w, static_cast<const float4 *>(d.records),
                                   static_cast<const SceneView *>(d.views), (const float *const *)table);
            else
                hipLaunchKernelGGL(instance_sign_kernel<false>, grid, dim3(kBlock), lds, stream, w, static_cast<const float4 *>(d.records),
                                   static_cast<const SceneView *>(d.views), (const float *const *)table);
            return launched("instanced signed-distance sign");
        });
    }
    const hipError_t e = hipFreeAsync(scratch, stream);
    if (rc)
        return rc;
    HIP_TRY(e);
    return SHRAY_OK;
}

// the blocking forms: the points to the device, the query on the null stream, the values, records, instances (and tallies)
// back
int signed_host(shray_instance_set *set, const shray_point *points, int64_t count, float *signed_out, shray_closest *closest,
                int32_t *instances, shray_counters *counters)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!set || !points || (!signed_out && !counters))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, points or signed is NULL");
    if (counters) {
        memset(counters, 0, sizeof(*counters));
        counters->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    if (const int rc = enter_set(set))   // (the errors of a set come before any allocation)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}},
                        {{signed_out, n * sizeof(float)}, {closest, closest ? n * sizeof(shray_closest) : 0}, {instances, instances ? n * sizeof(int32_t) : 0}},
                        counters, [&](DeviceBuffer *d_points, DeviceBuffer *d_out, DeviceCounters *shards) {
                            return signed_device(set, d_points->as<const shray_point>(), count, d_out[0].as<float>(), d_out[1].as<shray_closest>(),
                                                 d_out[2].as<int32_t>(), nullptr, shards);
                        });
}

}   // namespace

extern "C" {

int shray_signed_distance_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float *d_signed,
                                           shray_closest *d_closest, int32_t *d_instances, void *hip_stream)
{
    return signed_device(set, d_points, count, d_signed, d_closest, d_instances, (hipStream_t)hip_stream, nullptr);
}

int shray_signed_distance_instances(shray_instance_set *set, const shray_point *points, int64_t count, float *signed_out,
                                    shray_closest *closest, int32_t *instances)
{
    if (!signed_out && count > 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "signed is NULL");
    return signed_host(set, points, count, signed_out, closest, instances, nullptr);
}

int shray_signed_distance_instances_counters(shray_instance_set *set, const shray_point *points, int64_t count, float *signed_out,
                                             shray_closest *closest, int32_t *instances, shray_counters *counters)
{
    if (!counters)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
    return signed_host(set, points, count, signed_out, closest, instances, counters);
}

}   // extern "C"
