// TEST-ONLY: the exponential-map step, the damped 6x6 solve and the step measure of csrc/refine_core.h behind C entries for ctypes
// (tests/test_refine_core_shim.py).  The refinement only ever shows them through a converged pose; here they are held to properties
// of their own.
#include "../../cvxpnpl_amd/csrc/refine_core.h"

extern "C" {

// R [9] <- exp([d[0..3)]x) R, tc [3] <- tc + d[3..6)
void rf_pose_step(double *R, double *tc, const double *d)
{
    cvxr::Pose ps = {};
    for (int i = 0; i < 9; ++i) ps.R[i] = R[i];
    for (int i = 0; i < 3; ++i) ps.tc[i] = tc[i];
    cvxr::pose_step(ps, d);
    for (int i = 0; i < 9; ++i) R[i] = ps.R[i];
    for (int i = 0; i < 3; ++i) tc[i] = ps.tc[i];
}

// a [28]: the sums of an evaluation ([0,21) J^T J upper triangle row by row, [21,27) J^T r); d [6].  Returns cvxr::damped_step's bool.
int rf_damped_step(const double *a, double lambda, double *d) { return cvxr::damped_step(a, lambda, d) ? 1 : 0; }

// |step| in the public chart over (1 + |t|) at the pose (R, tc) about the centre c
double rf_step_measure(const double *R, const double *tc, const double *c, const double *d)
{
    cvxr::Pose ps = {};
    for (int i = 0; i < 9; ++i) ps.R[i] = R[i];
    for (int i = 0; i < 3; ++i) { ps.tc[i] = tc[i]; ps.c[i] = c[i]; }
    return cvxr::step_measure(ps, d);
}

} // extern "C"
