// instance_winding.hip -- include/shader_ray_instance_winding.h: winding numbers of world-space points over a set of placed
// scenes, each instance's term taken in its object space and signed by the orientation of its map, and the distance signed by
// their sum.
//
// orient_instances, one lane per instance, turns the set's current W rows into +-1.0f in stream-ordered scratch; every query
// runs it on its own stream, so it follows a device update enqueued there and there is no state to invalidate.
// wn_instances is one lane per point in one-wave workgroups.  Its loop over the instances is wave-uniform: every lane visits
// every instance in ascending order, so what a turn selects -- W's rows, the scene slot, the member's SceneView, the member's
// node-record pointer and the orientation -- arrives by scalar loads.  Each lane maps its point by the object ray's rule and
// runs winding/winding_walk.h's walk in its LDS stack column, adds the signed term and keeps the first containing instance.
// The SIGNED instance reads libshray_instance_point.so's records (its device form on the caller's stream, into the caller's
// buffer or stream-ordered scratch), walks only for hits and writes the signed distance.
// The node records belong to libshray_winding.so, which hands out each member scene's pointer, current on the stream
// (shrayi_scene_winding_records).  The per-slot table of those pointers reaches the device as launch arguments, as
// instance_sdf/instance_sdf.hip's does; the helper is a copy of this library's own, so that library's code object stays as
// it is.  Nothing of the two libraries' kernels is compiled here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "client_internal.h"
#include "enter_set.h"
#include "packed_walk.h"
#include "shader_ray_instance_winding.h"
#include "top_level.h"
#include "trace_common.h"
#include "winding_walk.h"

using namespace shray;

// libshray_winding.so's, outside its header: a scene's node records on its device, current for work enqueued on `hip_stream`
// after the call (derived there when stale).  Host-only; blocks only for the topology readback of a scene's first use.
extern "C" int shrayi_scene_winding_records(shray_scene *scene, void *hip_stream, const float **d_records);

namespace {

constexpr uint64_t kChunk = 1ull << 22;   // points per scratch chunk when the caller keeps no records
constexpr int kSlotsPerLaunch = 256;      // node-record pointers one table launch carries in its arguments (2 KiB)
constexpr int kOrientBlock = 256;

struct RecordSlots {
    const float *records[kSlotsPerLaunch];
};

// The per-slot table of node-record pointers reaches the device as a launch's arguments: stream-ordered, with no staging
// memory whose lifetime the host would have to watch.
__global__ void __launch_bounds__(kSlotsPerLaunch) store_record_slots(const float **table, RecordSlots slots, int n)
{
    if ((int)threadIdx.x < n)
        table[threadIdx.x] = slots.records[threadIdx.x];
}

// One lane per instance: the header's determinant of W's linear part in double (a product of two floats is exact there; the
// rest rounds once per operation, left to right), stored as its sign.
__global__ void __launch_bounds__(kOrientBlock) orient_instances(const float4 *__restrict__ set_records, int32_t count, float *__restrict__ orient)
{
    const int32_t i = (int32_t)(blockIdx.x * kOrientBlock + threadIdx.x);
    if (i >= count)
        return;
    const float4 r0 = set_records[4u * (uint32_t)i], r1 = set_records[4u * (uint32_t)i + 1u], r2 = set_records[4u * (uint32_t)i + 2u];
    const double w00 = r0.x, w01 = r0.y, w02 = r0.z, w10 = r1.x, w11 = r1.y, w12 = r1.z, w20 = r2.x, w21 = r2.y, w22 = r2.z;
    const double det = w00 * (w11 * w22 - w12 * w21) - w01 * (w10 * w22 - w12 * w20) + w02 * (w10 * w21 - w11 * w20);
    orient[i] = det < 0.0 ? -1.0f : 1.0f;
}

struct WnWork {
    const float4 *points;       // (p, max_dist2), world space
    const float4 *records;      // SIGNED: stage 1's, 2 per point
    float *out;                 // the winding numbers, or SIGNED: the signed distances
    int32_t *containing;        // one per point, or nullptr
    uint64_t count;
    uint64_t first;             // this launch's first point
    int32_t instance_count;
    float beta;
};

// One lane per point (file comment).  The set's records, the views, the table and the orientations are __restrict__ so that
// what a turn of the instance loop selects comes in by scalar loads.
template <bool SIGNED>
__global__ void __launch_bounds__(kBlock) wn_instances(WnWork w, const float4 *__restrict__ set_records, const SceneView *__restrict__ views,
                                                       const float *const *__restrict__ records_of_slot, const float *__restrict__ orient)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t wstack[];
    uint32_t *column = wstack + threadIdx.x;
    const uint64_t index = w.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = index < w.count;
    float4 in = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float dist2 = 0.0f;
    bool walks = live;
    if (live) {
        in = w.points[index];
        if (SIGNED) {
            dist2 = w.records[2 * index].w;
            walks = __float_as_int(w.records[2 * index + 1].z) >= 0;   // a hit (its point is finite); a miss is NaN with no walk
        } else {
            walks = __builtin_isfinite(in.x) && __builtin_isfinite(in.y) && __builtin_isfinite(in.z);
        }
    }
    const V3 pw = mk(in.x, in.y, in.z);
    float sum = 0.0f;
    int first_in = -1;
    if (__builtin_amdgcn_ballot_w64(walks)) {
        for (int32_t i = 0; i < w.instance_count; i++) {
            // wave-uniform: scalar loads
            const float4 *rec = set_records + 4u * (uint32_t)i;
            const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
            const uint32_t slot = __float_as_uint(rec[3].x);
            const SceneView &sc = views[slot];
            const WindingView v{reinterpret_cast<const float4 *>(records_of_slot[slot]),
                                static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes, sc.positions, sc.packed_root,
                                w.beta};
            const float s = orient[i];
            if (walks) {
                const V3 po = mk(object_row(w0, pw, true), object_row(w1, pw, true), object_row(w2, pw, true));
                // shray_winding_number's value for {p_o}: NaN for a non-finite coordinate, else the walk's
                const bool finite = __builtin_isfinite(po.x) && __builtin_isfinite(po.y) && __builtin_isfinite(po.z);
                const float wi = finite ? winding_walk(v, po, column) : __uint_as_float(0x7fc00000u);
                const float t = s < 0.0f ? -wi : wi;
                sum = sum + t;
                if (first_in < 0 && t > 0.5f)
                    first_in = i;
            }
        }
    }
    if (!live)
        return;
    if (SIGNED) {
        const float d = sqrtf(dist2);
        w.out[index] = !walks ? __uint_as_float(0x7fc00000u) : (sum > 0.5f && dist2 > 0.0f) ? -d : d;
    } else {
        w.out[index] = walks ? sum : __uint_as_float(0x7fc00000u);
        if (w.containing)
            w.containing[index] = first_in;
    }
}

// every distinct member scene's node records current on `stream`, and the table of their pointers, by scene slot, written
// to `table` in stream order
int stage_record_slots(const ShrayInstanceSetDevice &d, const float **table, hipStream_t stream)
{
    for (int32_t base = 0; base < d.scene_count; base += kSlotsPerLaunch) {
        const int n = std::min<int32_t>(kSlotsPerLaunch, d.scene_count - base);
        RecordSlots slots;
        memset(&slots, 0, sizeof(slots));
        for (int k = 0; k < n; k++)
            if (const int rc = shrayi_scene_winding_records(d.scenes[base + k], stream, &slots.records[k]))
                return rc;
        hipLaunchKernelGGL(store_record_slots, dim3(1), dim3(kSlotsPerLaunch), 0, stream, table + base, slots, n);
        if (const int rc = launched("instanced winding record table"))
            return rc;
    }
    return SHRAY_OK;
}

int enqueue_orientations(const ShrayInstanceSetDevice &d, float *orient, hipStream_t stream)
{
    hipLaunchKernelGGL(orient_instances, dim3(grid_of((uint64_t)d.count, kOrientBlock)), dim3(kOrientBlock), 0, stream,
                       static_cast<const float4 *>(d.records), d.count, orient);
    return launched("instance orientations");
}

// the refusals of both device forms, before any device is touched
int check_query(shray_instance_set *set, const void *points, int64_t count, float beta, const void *out)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative point count %lld", (long long)count);
    if (!set || !points || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set, points or out is NULL");
    if (!(beta >= 0.0f))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "beta is %g: it must be >= 0 (+INFINITY: exact)", (double)beta);
    return SHRAY_OK;
}

// Both device forms: d_signed null is the winding number's (d_out, d_containing), else the winding-signed distance's
// (d_signed, d_closest, d_instances).
int query_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta, float *d_out, int32_t *d_containing,
                 float *d_signed, shray_closest *d_closest, int32_t *d_instances, hipStream_t stream)
{
    const bool with_sign = d_signed != nullptr;
    if (count == 0)
        return SHRAY_OK;
    ShrayInstanceSetDevice d;
    int height = 0;
    int rc = enter_set(set, &d, &height);   // (a member tree that is too high is refused here, before any launch)
    if (rc)
        return rc;
    const uint64_t n = (uint64_t)count;
    // scratch, stream-ordered: the table, the orientations, and the records of at most kChunk points the caller does not keep
    const uint64_t chunk = !with_sign || d_closest ? n : std::min(n, kChunk);
    const size_t table_bytes = (size_t)d.scene_count * sizeof(const float *);
    const size_t orient_at = (table_bytes + 255) & ~(size_t)255;
    const size_t records_at = (orient_at + (size_t)d.count * sizeof(float) + 255) & ~(size_t)255;
    const size_t total = records_at + (with_sign && !d_closest ? chunk * sizeof(shray_closest) : 0);
    char *scratch = nullptr;
    HIP_TRY(hipMallocAsync((void **)&scratch, total, stream));
    const float **table = reinterpret_cast<const float **>(scratch);
    float *orient = reinterpret_cast<float *>(scratch + orient_at);
    rc = stage_record_slots(d, table, stream);
    if (!rc)
        rc = enqueue_orientations(d, orient, stream);
    const size_t lds = (size_t)kBlock * stack_levels(height) * sizeof(uint32_t);   // a lane's column: one word per level of the tallest member
    for (uint64_t first = 0; first < n && !rc; first += chunk) {
        const uint64_t m = std::min(chunk, n - first);
        shray_closest *records = nullptr;
        if (with_sign) {
            records = d_closest ? d_closest + first : reinterpret_cast<shray_closest *>(scratch + records_at);
            rc = shray_closest_points_instances_device(set, d_points + first, (int64_t)m, records, d_instances ? d_instances + first : nullptr, stream);
            if (rc)
                break;
        }
        WnWork w{(const float4 *)(d_points + first), (const float4 *)records, (with_sign ? d_signed : d_out) + first,
                 d_containing ? d_containing + first : nullptr, m, 0, d.count, beta};
        rc = for_each_launch((m + kBlock - 1) / kBlock, kPointsPerLaunch / kBlock, [&](uint64_t first_block, dim3 grid) {
            w.first = first_block * kBlock;
            if (with_sign)
                hipLaunchKernelGGL(wn_instances<true>, grid, dim3(kBlock), lds, stream, w, static_cast<const float4 *>(d.records),
                                   static_cast<const SceneView *>(d.views), (const float *const *)table, (const float *)orient);
            else
                hipLaunchKernelGGL(wn_instances<false>, grid, dim3(kBlock), lds, stream, w, static_cast<const float4 *>(d.records),
                                   static_cast<const SceneView *>(d.views), (const float *const *)table, (const float *)orient);
            return launched("instanced winding number");
        });
    }
    const hipError_t e = hipFreeAsync(scratch, stream);
    if (rc)
        return rc;
    HIP_TRY(e);
    return SHRAY_OK;
}

int number_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta, float *d_out, int32_t *d_containing,
                  hipStream_t stream)
{
    if (const int rc = check_query(set, d_points, count, beta, d_out))
        return rc;
    if (!aligned(d_points, 16) || !aligned(d_out, 4) || !aligned(d_containing, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "the point buffer must be 16-byte aligned, the values and the containing instances 4-byte aligned");
    return query_device(set, d_points, count, beta, d_out, d_containing, nullptr, nullptr, nullptr, stream);
}

int signed_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta, float *d_signed, shray_closest *d_closest,
                  int32_t *d_instances, hipStream_t stream)
{
    if (const int rc = check_query(set, d_points, count, beta, d_signed))
        return rc;
    if (!aligned(d_points, 16) || !aligned(d_closest, 16) || !aligned(d_signed, 4) || !aligned(d_instances, 4))
        return fail(SHRAY_ERR_INVALID_ARGUMENT,
                    "point and record buffers must be 16-byte aligned, the signed values and the instance buffer 4-byte aligned");
    return query_device(set, d_points, count, beta, nullptr, nullptr, d_signed, d_closest, d_instances, stream);
}

}   // namespace

extern "C" {

int shray_winding_number_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta, float *d_out,
                                          int32_t *d_containing, void *hip_stream)
{
    return number_device(set, d_points, count, beta, d_out, d_containing, (hipStream_t)hip_stream);
}

// the points to the device, the device form on the null stream, the values (and containing instances) back
int shray_winding_number_instances(shray_instance_set *set, const shray_point *points, int64_t count, float beta, float *out,
                                   int32_t *containing)
{
    int rc = check_query(set, points, count, beta, out);
    if (rc || count == 0)
        return rc;
    if ((rc = enter_set(set)))   // (the errors of a set come before any allocation)
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}}, {{out, n * sizeof(float)}, {containing, containing ? n * sizeof(int32_t) : 0}}, nullptr,
                        [&](DeviceBuffer *d_in, DeviceBuffer *d_out, DeviceCounters *) {
                            return number_device(set, d_in[0].as<const shray_point>(), count, beta, d_out[0].as<float>(), d_out[1].as<int32_t>(),
                                                 nullptr);
                        });
}

int shray_winding_signed_distance_instances_device(shray_instance_set *set, const shray_point *d_points, int64_t count, float beta,
                                                   float *d_signed, shray_closest *d_closest, int32_t *d_instances, void *hip_stream)
{
    return signed_device(set, d_points, count, beta, d_signed, d_closest, d_instances, (hipStream_t)hip_stream);
}

int shray_winding_signed_distance_instances(shray_instance_set *set, const shray_point *points, int64_t count, float beta, float *signed_out,
                                            shray_closest *closest, int32_t *instances)
{
    int rc = check_query(set, points, count, beta, signed_out);
    if (rc || count == 0)
        return rc;
    if ((rc = enter_set(set)))
        return rc;
    const size_t n = (size_t)count;
    return run_blocking({{points, n * sizeof(shray_point)}},
                        {{signed_out, n * sizeof(float)}, {closest, closest ? n * sizeof(shray_closest) : 0}, {instances, instances ? n * sizeof(int32_t) : 0}},
                        nullptr, [&](DeviceBuffer *d_in, DeviceBuffer *d_out, DeviceCounters *) {
                            return signed_device(set, d_in[0].as<const shray_point>(), count, beta, d_out[0].as<float>(),
                                                 d_out[1].as<shray_closest>(), d_out[2].as<int32_t>(), nullptr);
                        });
}

int shray_instance_set_orientations(shray_instance_set *set, float *out)
{
    if (!set || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or out is NULL");
    ShrayInstanceSetDevice d;
    int rc = shrayi_instance_set_device_arrays(set, &d);
    if (rc || (rc = use_device(d.device)))
        return rc;
    if (d.count <= 0)
        return SHRAY_OK;
    DeviceBuffer orient;
    HIP_TRY(orient.alloc((size_t)d.count * sizeof(float)));
    if ((rc = enqueue_orientations(d, orient.as<float>(), nullptr)))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out, orient.p, (size_t)d.count * sizeof(float), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

}   // extern "C"
