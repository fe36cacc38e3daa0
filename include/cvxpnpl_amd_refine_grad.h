/*
 * cvxpnpl_amd_refine_grad.h -- C ABI of the backward pass of the reprojection refinement (libcvxpnpl_amd_refine_grad.so).
 *
 * The sixth library, beside the solver's, its backward pass's, the two RANSAC libraries and the refinement's: none of them depends on it,
 * and its kernels are held against a resource table of their own (tests/golden/refine_grad_kernel_resources.json).  Same conventions as
 * the other ABIs: plain pointers and sizes, contiguous float64 arrays, DEVICE pointers on the current device unless stated otherwise.
 *
 * What it computes.  A converged refinement (cvxpnpl_amd_refine.h) is a strict local minimum of
 * f = 1/2 sum rho^2 over the pixel residuals of the LIVE correspondences, so the implicit function theorem gives the vector-Jacobian
 * product dL/d(pts_2d, pts_3d, line_2d, line_3d) from dL/dR and dL/dt through one 6x6 solve per problem with the FULL Hessian of f
 * (Gauss-Newton term plus residual-weighted second derivatives) and one pass over the records.  Nothing of the iteration is
 * differentiated.  K gets no gradient; the pose handed in gets none either: a minimiser does not depend on where the iteration started.
 * Residuals, liveness (mask byte absent or non-zero; a line only when a != b) and layouts are those of cvxpnpl_amd_refine.h.  The
 * upstream gradients are taken in the chart R' = exp([w]x) R, t' = t + tau:  b = (axial vector of G_R R^T - R G_R^T,  g_t).
 * All arithmetic float64.
 */
#ifndef CVXPNPL_AMD_REFINE_GRAD_H
#define CVXPNPL_AMD_REFINE_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CVXPNPL_REFINE_VJP_OK = 0,       /* differentiated */
    CVXPNPL_REFINE_VJP_SKIPPED = 1,  /* refine status not in admit_mask, a non-finite pose, or det R <= 0 */
    CVXPNPL_REFINE_VJP_SINGULAR = 2, /* fewer than 3 live correspondences, or H not positive definite: the pose is not a strict minimum */
    CVXPNPL_REFINE_VJP_BEHIND = 3    /* a live record has depth <= 0 or holds a number that is not finite (or an upstream gradient does) */
};
/* For statuses 1-3 every gradient of the problem is zero.  Every element of every gradient array that is passed is written: zeros for
 * records that are not live and for problems that are not differentiated. */

/*
 * Batch form: the arguments of cvxpnpl_refine_batch where the meaning is the same (layouts, K shared or per problem, masks).
 *   d_R, d_t                 the poses to differentiate at: the outputs of the refinement
 *   d_refine_status, status_stride   optional: the refinement's status column, problem b reads d_refine_status[b * status_stride]; NULL
 *                            means every problem.  admit_mask: bit s set = refine status s is differentiated (1 = CONVERGED only)
 *   d_grad_R [batch][9], d_grad_t [batch][3]   the upstream gradients; either may be NULL (zero)
 * outputs: d_g_pts_2d [batch][n_p][2], d_g_pts_3d [batch][n_p][3], d_g_line_2d [batch][n_l][2][2], d_g_line_3d [batch][n_l][2][3]: any may
 *   be NULL (not wanted); d_vjp_status [batch] int32; d_info [batch][2] (optional): |g| / sum |J| |rho| -- the stationarity of the pose
 *   handed in, where a pose stopped by max_iters shows -- and the smallest ratio L_jj^2 / H_jj of the Cholesky factorisation of H; NaN
 *   for a problem whose sums were not taken to the end (statuses 1 and 3, fewer than 3 live).
 * 16 lanes per problem, one launch.  Asynchronous on `stream`.  Returns 0, -1 bad arguments (nothing is launched), -2 HIP error.
 * batch = 0 is a no-op.
 */
int cvxpnpl_refine_vjp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                             const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                             const int32_t *d_refine_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                             const uint8_t *d_mask_lines, const double *d_grad_R, const double *d_grad_t, double *d_g_pts_2d, double *d_g_pts_3d,
                             double *d_g_line_2d, double *d_g_line_3d, int32_t *d_vjp_status, double *d_info, void *stream);

/* The same on the host: HOST pointers, n_threads host threads (<= 0: all cores) instead of a stream; the same source
 * (refine_vjp_core.h) as the kernels.  Returns 0, or -1 for bad arguments. */
int cvxpnpl_refine_vjp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                  const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                  const int32_t *refine_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                  const uint8_t *mask_lines, const double *grad_R, const double *grad_t, double *g_pts_2d, double *g_pts_3d,
                                  double *g_line_2d, double *g_line_3d, int32_t *vjp_status, double *info, int32_t n_threads);

/*
 * Packed scenes, the layout of cvxpnpl_refine_scenes (offsets clamped to the packed arrays, d_ln_offsets may be NULL when n_lines is 0);
 * one pose, one upstream gradient, one status per scene.  The gradients are in the packed layouts d_g_pts_2d [n_pts][2], d_g_pts_3d
 * [n_pts][3], d_g_line_2d [n_lines][2][2], d_g_line_3d [n_lines][2][3]; a scene writes the records of its own slices.  One workgroup per
 * scene, one launch.  n_scenes = 0 is a no-op.
 */
int cvxpnpl_refine_vjp_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                              const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                              int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_refine_status, int64_t status_stride,
                              uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_grad_R,
                              const double *d_grad_t, double *d_g_pts_2d, double *d_g_pts_3d, double *d_g_line_2d, double *d_g_line_3d,
                              int32_t *d_vjp_status, double *d_info, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_refine_grad_last_error(void);

const char *cvxpnpl_refine_grad_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_REFINE_GRAD_H */
