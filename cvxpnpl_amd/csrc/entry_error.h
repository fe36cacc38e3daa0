// entry_error.h -- the error text of a library's entry points: the thread-local message behind its *_last_error, the -1 of a bad argument
// and the -2 of a failed HIP call.  Shared by solver_entry.h, refine_entry.h and ransac_entry.h.  Host-only, plain C++17; what needs the
// HIP runtime is behind __HIPCC__.  Every function is inline and hidden: each library keeps a copy of its own -- its own message -- and
// exports nothing of this.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#define CVXEE_FN inline __attribute__((visibility("hidden")))

namespace cvxee {

CVXEE_FN char *err_buf()
{
    static thread_local char buf[512] = "";
    return buf;
}

// a free-form message, and the code the entry point returns with it
CVXEE_FN __attribute__((format(printf, 2, 3))) int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

CVXEE_FN int bad_args(const char *who, const char *what)
{
    snprintf(err_buf(), 512, "%s: bad arguments (%s)", who, what);
    return -1;
}

#if defined(__HIPCC__)
// a HIP call that failed (an allocation, a query, an event: not only a launch)
CVXEE_FN int hip_error(const char *what, hipError_t e)
{
    snprintf(err_buf(), 512, "%s: %s", what, hipGetErrorString(e));
    return -2;
}

CVXEE_FN int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_error(what, e);
}
#endif

} // namespace cvxee
