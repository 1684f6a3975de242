// error_internal.h -- how libshray_hip.so and its client libraries (libshray_query.so, libshray_refit.so, libshray_instance.so,
// libshray_point.so) report an error: the message goes to shray_last_error() (capi.hip keeps it, per thread) and the code is
// returned; and the device switch their entry points begin with, which reports its failure that way.  Host-only, internal to
// the libraries; not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "shader_ray_hip.h"

extern "C" int shrayi_fail(int code, const char *message);   // capi.hip: sets shray_last_error(), returns `code`

namespace {

// shrayi_fail with a printf-style message (cut at 511 characters)
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return shrayi_fail(code, buf);
}

}   // namespace

// a failed HIP call returns SHRAY_ERR_OUT_OF_MEMORY or SHRAY_ERR_DEVICE, naming the call
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? SHRAY_ERR_OUT_OF_MEMORY : SHRAY_ERR_DEVICE, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                                        \
    } while (0)

namespace {

// `device` made current unless it is (a scene's or a set's buffers live on its device)
inline int use_device(int device)
{
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != device)
        HIP_TRY(hipSetDevice(device));
    return SHRAY_OK;
}

}   // namespace
