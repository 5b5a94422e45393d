// mrt_err.h — the error state behind mrt_last_error / mrt_last_status, as every host unit of the library sets it.  No HIP here:
// mrt_image_io.cpp includes this header alone; the units that talk to the device get it through mrt_ctx.h.
#pragma once
#include <string>

#include "../../include/mrt.h"

namespace mrt {
namespace api {

// per thread, like errno: a thread-per-connection server reads its own call's error (defined in mrt_api.cpp)
extern thread_local std::string g_err;
extern thread_local int g_status;

int fail(int code, const char *fmt, ...);
inline void ok() { g_status = MRT_OK; }

// an error path that still waits for work already launched: the caller gets the first error, rc, whatever `cleanup` runs into
template <class F> int keep_first_error(int rc, F &&cleanup)
{
    const std::string keep = g_err;
    cleanup();
    g_err = keep; g_status = rc;
    return rc;
}

}  // namespace api
}  // namespace mrt
