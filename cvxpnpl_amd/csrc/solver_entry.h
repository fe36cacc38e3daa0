// solver_entry.h -- what the entry points of the solver library (cvxpnpl_hip.hip) and of the pose-VJP library (grad_hip.hip) share around
// their kernels: the error text, the contract of a correspondence block and the limit of one launch.  Host-only.  Every function is inline
// and hidden: each library keeps a copy of its own -- its own thread-local message -- and exports nothing of this.
#pragma once
#include <stdint.h>

#include "entry_error.h"

#define CVXSE_FN inline __attribute__((visibility("hidden")))

namespace cvxse {

// the error text: entry_error.h
using cvxee::err_buf;
using cvxee::fail;
using cvxee::hip_error;
using cvxee::launched;

// The correspondence block of an entry point -- batch, n_p points, n_l lines, K: no negative size, K given, and both halves of every kind
// that has records.  (Whether a call without any record is one too is the entry point's: the solves, the assemblies and the VJP refuse it,
// the generator does not.)
CVXSE_FN bool bad_corr_block(int64_t batch, int32_t n_p, const void *p2, const void *p3, int32_t n_l, const void *l2, const void *l3, const void *K)
{
    return batch < 0 || n_p < 0 || n_l < 0 || !K || (n_p > 0 && (!p2 || !p3)) || (n_l > 0 && (!l2 || !l3));
}

// one launch holds this many blocks along x; over_grid: the refusal of a larger one, in the entry point's words
constexpr int64_t GRID_MAX = 0x7fffffffLL;

CVXSE_FN int over_grid(int64_t grid, const char *msg) { return grid > GRID_MAX ? fail(-1, "%s", msg) : 0; }

} // namespace cvxse
