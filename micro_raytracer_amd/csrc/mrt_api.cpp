// mrt_api.cpp — the C ABI of include/mrt.h: context management, uploads, launches, read-back.
// Replaces the reference's Sampler (src/sampler.rs:11-100); there is no CPU rendering path here:
// without a HIP device every entry point that needs one fails with MRT_ERR_DEVICE.
// This unit: the error state and the entry points that need no context.  The rest of the ABI, by feature: mrt_create.cpp,
// mrt_execute.cpp, mrt_adaptive.cpp, mrt_accum.cpp, mrt_aov.cpp, mrt_radiance.cpp, mrt_hooks.cpp (mrt_ctx.h: what they share).
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdio.h>

#include "mrt_err.h"

namespace mrt {
namespace api {

thread_local std::string g_err;
thread_local int g_status = MRT_OK;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    g_status = code;
    return code;
}

}  // namespace api
}  // namespace mrt

using namespace mrt::api;

extern "C" {

uint32_t mrt_abi_version(void) { return MRT_ABI_VERSION; }
const char *mrt_last_error(void) { return g_err.c_str(); }
int mrt_last_status(void) { return g_status; }

int mrt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
