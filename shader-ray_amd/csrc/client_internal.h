// client_internal.h -- the host-side scaffolding that the client libraries of libshray_hip.so (query/, refit/, instance/,
// point/) share: an owning device allocation, the device switch, the launch check, the split of a large launch and the blocking
// form of a query.  Host-only, internal to the libraries; not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "counters_internal.h"
#include "device_types.h"
#include "error_internal.h"
#include "scene_access_internal.h"

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

// `device` made current unless it is (a scene's or a set's buffers live on its device)
inline int use_device(int device)
{
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != device)
        HIP_TRY(hipSetDevice(device));
    return SHRAY_OK;
}

// the scene's query view, on its device
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

}   // namespace
