// client_internal.h -- the host-side scaffolding that the client libraries of libshray_hip.so (query/, refit/, instance/,
// point/, sdf/, winding/, multihit/, near/, overlap/, instance_multihit/) share: an owning device allocation, the device switch, the
// launch check and the grid of a launch, the split of a large launch, the blocking form of a query, the upload of a tree's
// height order (tree_order.h) and the bookkeeping of what a library derives from a scene's geometry (DerivedState).  What the
// counted, first-K queries share on top of it (multihit/, instance_multihit/, near/, overlap/) is point/first_k_query.h.
// Host-only, internal to the libraries; not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "counters_internal.h"
#include "device_types.h"
#include "error_internal.h"
#include "scene_access_internal.h"
#include "tree_order.h"

namespace {

// One owning device allocation, freed when it goes out of scope.
struct DeviceBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer()
    {
        if (p)
            (void)hipFree(p);
    }
    // `n` bytes for a new buffer, 16 for none (a valid pointer even for an empty array)
    hipError_t alloc(size_t n) { return grow(n ? n : 16); }
    // at least `want` bytes: what is there when it is large enough, else a new allocation (the contents are not kept)
    hipError_t grow(size_t want)
    {
        if (want <= bytes)
            return hipSuccess;
        if (p)
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess)
            bytes = want;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

inline bool aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1u)) == 0; }

// the scene's query view, on its device (use_device: error_internal.h)
inline int enter_scene(shray_scene *scene, ShrayQueryScene *q)
{
    if (!scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "scene is NULL");
    const int rc = shrayi_scene_query_view(scene, q);
    return rc ? rc : use_device(q->device);
}

// the check after a launch, naming it
inline int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SHRAY_OK : fail(SHRAY_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
}

// workgroups of `block` threads for `items` threads
inline unsigned int grid_of(uint64_t items, int block) { return (unsigned int)((items + block - 1) / block); }

// `blocks` workgroups in launches of at most `per_launch`: launch(first block, grid) for each, up to the first error
template <typename Launch>
int for_each_launch(uint64_t blocks, uint64_t per_launch, Launch &&launch)
{
    for (uint64_t first = 0; first < blocks; first += per_launch) {
        const int rc = launch(first, dim3((unsigned int)(blocks - first < per_launch ? blocks - first : per_launch)));
        if (rc)
            return rc;
    }
    return SHRAY_OK;
}

// host memory a blocking form stages on the device, and host memory it returns (host null: computed, not returned; bytes 0:
// not allocated, the device pointer is null)
struct HostIn {
    const void *host;
    size_t bytes;
};
struct HostOut {
    void *host;
    size_t bytes;
};

// The blocking form of a query: the inputs to the device, `enqueue(inputs, outputs, shards)` (the device form, on the null
// stream), then the outputs back, and the tallies into *counters when it is not null (shards is null otherwise).
template <size_t NI, size_t NO, typename Enqueue>
int run_blocking(const HostIn (&in)[NI], const HostOut (&out)[NO], shray_counters *counters, Enqueue &&enqueue)
{
    DeviceBuffer d_in[NI], d_out[NO], shards;
    for (size_t k = 0; k < NI; k++)
        HIP_TRY(d_in[k].alloc(in[k].bytes));
    for (size_t k = 0; k < NO; k++)
        if (out[k].bytes)
            HIP_TRY(d_out[k].alloc(out[k].bytes));
    if (counters) {
        HIP_TRY(shards.alloc(sizeof(shray::DeviceCounters) * shray::kCounterShards));
        HIP_TRY(hipMemset(shards.p, 0, shards.bytes));
    }
    for (size_t k = 0; k < NI; k++)
        HIP_TRY(hipMemcpy(d_in[k].p, in[k].host, in[k].bytes, hipMemcpyHostToDevice));
    const int rc = enqueue(d_in, d_out, shards.as<shray::DeviceCounters>());
    if (rc)
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < NO; k++)
        if (out[k].host && out[k].bytes)
            HIP_TRY(hipMemcpy(out[k].host, d_out[k].p, out[k].bytes, hipMemcpyDeviceToHost));
    return counters ? sum_counter_shards(shards.as<const shray::DeviceCounters>(), counters) : SHRAY_OK;
}

// A TreeOrder on the device, as the bottom-up kernels read it: `order`, `topo` (per node) and `heights` (height_start).
struct DeviceTreeOrder {
    DeviceBuffer order, topo, heights;
};

// `t`'s arrays onto the device and released on the host: by blocking copies, or by copies enqueued on `stream` and one
// synchronisation of it
inline int upload_tree_order(TreeOrder &t, DeviceTreeOrder &d, bool blocking, hipStream_t stream)
{
    const auto put = [&](DeviceBuffer &to, const void *from, size_t bytes) {
        HIP_TRY(to.alloc(bytes));
        HIP_TRY(blocking ? hipMemcpy(to.p, from, bytes, hipMemcpyHostToDevice) : hipMemcpyAsync(to.p, from, bytes, hipMemcpyHostToDevice, stream));
        return (int)SHRAY_OK;
    };
    int rc = put(d.order, t.order.data(), t.order.size() * sizeof(uint32_t));
    rc = rc ? rc : put(d.topo, t.topo.data(), t.topo.size() * sizeof(Topo));
    rc = rc ? rc : put(d.heights, t.height_start.data(), t.height_start.size() * sizeof(uint32_t));
    if (!rc && !blocking)
        HIP_TRY(hipStreamSynchronize(stream));
    std::vector<uint32_t>().swap(t.order);   // (the schedule needs height_start and the counts only)
    std::vector<Topo>().swap(t.topo);
    return rc;
}

// What a library derives on the device from a scene's geometry (the signed distance's sign data, the winding number's node
// records) is current when `derived` is set and `generation` is the scene's geometry generation (scene_access_internal.h: a
// refit bumps it).  `done` is recorded after every derivation: other streams and the blocking calls wait on it.
struct DerivedState {
    bool derived = false;
    uint64_t generation = 0;
    hipEvent_t done = nullptr;
    DerivedState() { (void)hipEventCreateWithFlags(&done, hipEventDisableTiming); }   // (make_current reports a failure)
    ~DerivedState()
    {
        if (done)
            (void)hipEventDestroy(done);
    }
};

// What `st` derives made current on `stream`: when it is stale, derive() enqueued there and the event recorded after it;
// else `stream` waits for the event of the derivation, which may have run on another stream (no host synchronisation
// either way).  A derivation that fails leaves the state stale.
template <typename Derive>
int make_current(DerivedState &st, uint64_t generation, hipStream_t stream, Derive &&derive)
{
    if (!st.done)
        return fail(SHRAY_ERR_DEVICE, "the event that orders a scene's derived data could not be created");
    if (st.derived && st.generation == generation) {
        HIP_TRY(hipStreamWaitEvent(stream, st.done, 0));
        return SHRAY_OK;
    }
    st.derived = false;
    if (const int rc = derive())
        return rc;
    HIP_TRY(hipEventRecord(st.done, stream));
    st.derived = true;
    st.generation = generation;
    return SHRAY_OK;
}

}   // namespace
