// entry_error.h -- the error text of a library's entry points: the thread-local message behind its *_last_error, the -1 of a bad argument
// and the -2 of a failed launch.  Shared by refine_entry.h and ransac_entry.h.  Host-only, plain C++17; what needs the HIP runtime is
// behind __HIPCC__.  Every function is inline and hidden: each library keeps a copy of its own -- its own message -- and exports nothing
// of this.
#pragma once
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

CVXEE_FN int bad_args(const char *who, const char *what)
{
    snprintf(err_buf(), 512, "%s: bad arguments (%s)", who, what);
    return -1;
}

#if defined(__HIPCC__)
CVXEE_FN int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(err_buf(), 512, "%s: %s", what, hipGetErrorString(e));
    return -2;
}
#endif

} // namespace cvxee
