// device_array_check.h -- the check an asynchronous entry point makes of a caller's device array before it enqueues anything
// that reads it (libshray_refit.so, libshray_instance.so).  Host-only, internal to the libraries; not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "error_internal.h"

namespace {

// A device-path array must be device memory of `device` whose allocation holds all `bytes` of it: a host pointer (a CPU
// tensor, a numpy buffer) or a buffer on another GPU would be read by a kernel itself, and a short buffer read past its end.
// `owner` names what `device` belongs to in the message ("scene", "set").
int check_device_array(const void *p, size_t bytes, int device, const char *what, const char *owner)
{
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();     // (an unknown pointer is an answer here, not an error for the calls after this one)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s is not device memory (hipPointerGetAttributes: %s)", what, hipGetErrorString(e));
    }
    if (attr.type != hipMemoryTypeDevice || attr.device != device)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s is not device memory of the %s's device %d (memory type %d, device %d)", what,
                    owner, device, (int)attr.type, attr.device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s: its allocation is unknown", what);
    }
    if ((const char *)p + bytes > (const char *)base + size)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s: %zu bytes from it run past the end of its allocation", what, bytes);
    return SHRAY_OK;
}

}   // namespace
