/*
 * cvxpnpl_amd_grad.h -- C ABI of the backward pass of the batched pose solves (libcvxpnpl_amd_grad.so).
 *
 * A library of its own beside libcvxpnpl_amd.so: the solves (include/cvxpnpl_amd.h) do not depend on it, and its kernels are held
 * against a resource table of their own (tests/golden/grad_kernel_resources.json).  Same conventions as the solver's ABI: plain
 * pointers and sizes, contiguous problem-major float64 arrays, DEVICE pointers on the current device unless stated otherwise.
 */
#ifndef CVXPNPL_AMD_GRAD_H
#define CVXPNPL_AMD_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Gradients of a pose solve: the vector-Jacobian product of (R, t) with respect to the correspondences.
 * A certified pose is the global minimiser over O(3) x R^3 of the algebraic cost; at that point the first-order condition holds
 * and the implicit function theorem gives dL/d(correspondences) from one 6x6 solve per problem (float64 Cholesky), with the full
 * Hessian (not Gauss-Newton).  K is not differentiated.
 *   inputs      the layouts and pointers of cvxpnpl_solve_batch (d_pts_2d ... K_per_problem) and its outputs d_R [batch][9],
 *               d_t [batch][3], d_status [batch] (NULL: every problem is differentiated)
 *   admit_mask  bit s set: problems of status s are differentiated (1 << CVXPNPL_CERTIFIED, the default; 0x15: every rank-1 pose,
 *               CERTIFIED | UNCERTIFIED | REFLECTION, whose gradient is then that of the nearest stationary point's local model)
 *   d_gR [batch][9], d_gt [batch][3]   upstream gradients dL/dR (row-major), dL/dt; NULL = zero.  The component of d_gR normal to
 *               O(3) drops out.
 * outputs (NULL = not wanted, except d_vjp_status)
 *   d_g_pts_2d [batch][n_p][2], d_g_pts_3d [batch][n_p][3], d_g_line_2d [batch][n_l][2][2], d_g_line_3d [batch][n_l][2][3]
 *   d_vjp_status [batch] int32  CVXPNPL_VJP_*; every status other than OK writes zero gradients for its problem
 *   d_vjp_info [batch][2]       lambda_min(H) / lambda_max(H), and |g| / (2 sqrt(tr(H_gn) (f + 1e-20 scale))) -- how far the
 *                               pose is from stationary (<= 1; 0 at an exact minimiser); NaN for skipped problems
 * Small problems run 16 lanes per problem in one launch; from 768 records (points + 2 lines) a multi-workgroup reduction, a solve
 * and a scatter (three launches, stream-ordered scratch).  Asynchronous on `stream`.  Returns 0, -1 bad arguments, -2 HIP error (cvxpnpl_grad_last_error).
 */
enum {
    CVXPNPL_VJP_OK = 0,
    CVXPNPL_VJP_SKIPPED = 1,  /* status not in admit_mask */
    CVXPNPL_VJP_SINGULAR = 2, /* H not positive definite (a Cholesky pivot below 1e-11 of its diagonal entry): degenerate configuration;
                                 or fewer than three correspondences (n_p + n_l < 3: under six equations determine no pose) */
    CVXPNPL_VJP_NONFINITE = 3 /* NaN / inf in the pose, the inputs or the solve */
};
int cvxpnpl_pose_vjp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                           const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                           const int32_t *d_status, uint32_t admit_mask, const double *d_gR, const double *d_gt, double *d_g_pts_2d,
                           double *d_g_pts_3d, double *d_g_line_2d, double *d_g_line_3d, int32_t *d_vjp_status, double *d_vjp_info, void *stream);

/* The same on the host: HOST pointers, the same arguments, n_threads host threads (<= 0: all cores) instead of a stream; the same
 * source (vjp_core.h) as the device path.  Returns 0, or -1 for bad arguments. */
int cvxpnpl_pose_vjp_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                          const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                          const int32_t *status, uint32_t admit_mask, const double *gR, const double *gt, double *g_pts_2d,
                          double *g_pts_3d, double *g_line_2d, double *g_line_3d, int32_t *vjp_status, double *vjp_info, int32_t n_threads);

/* Message of the calling thread's last failed cvxpnpl_pose_vjp_batch ("" if none). */
const char *cvxpnpl_grad_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_GRAD_H */
