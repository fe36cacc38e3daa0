/*
 * cvxpnpl_amd_refine_robust_grad.h -- C ABI of the backward pass of the robust reprojection refinement
 * (libcvxpnpl_amd_refine_robust_grad.so).
 *
 * The eighth library, beside the seven others: none of them depends on it, and its kernels are held against a resource table of their
 * own (tests/golden/refine_robust_grad_kernel_resources.json).  Same conventions as the other ABIs: plain pointers and sizes, contiguous
 * float64 arrays, DEVICE pointers on the current device unless stated otherwise.
 *
 * What it computes.  A converged robust refinement (cvxpnpl_amd_refine_robust.h) is a strict local minimum of
 * F = 1/2 sum_k w_k rho(s_k) over the LIVE correspondences, so the implicit function theorem gives the vector-Jacobian product
 * dL/d(pts_2d, pts_3d, line_2d, line_3d, w_pts, w_lines) from dL/dR and dL/dt through one 6x6 solve per problem with the FULL Hessian
 * of F -- the Gauss-Newton term, the residual-weighted second derivatives and the rho'' term that the forward iteration drops -- and
 * one pass over the records.  Nothing of the iteration is differentiated.  K, scale_px and the pose handed in get no gradient.
 * Residuals, layouts, losses and liveness are those of cvxpnpl_amd_refine_robust.h: mask byte absent or non-zero, a line only when
 * a != b, and w_k != 0 -- a zero weight is a mask, the record behind it is not read, and its weight's gradient is exactly 0 (a
 * confidence that reaches 0 stays there).  The statuses, the upstream chart and `info` are those of cvxpnpl_amd_refine_grad.h.
 * All arithmetic float64.
 */
#ifndef CVXPNPL_AMD_REFINE_ROBUST_GRAD_H
#define CVXPNPL_AMD_REFINE_ROBUST_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vjp_status: 0 differentiated, 1 skipped, 2 fewer than 3 live correspondences or H not positive definite, 3 a live record behind the
 * camera or not finite, or a weight that is negative or not finite on a record its mask admits.  The checks come in that order: skipped,
 * bad weight, fewer than three live records, behind the camera or not finite.  For statuses 1-3 every gradient of the problem is zero.
 * Every element of every gradient array that is passed is written: zeros for records that are not live and for problems that are not
 * differentiated.
 *
 * loss: CVXPNPL_LOSS_L2 0, CVXPNPL_LOSS_HUBER 1, CVXPNPL_LOSS_CAUCHY 2 (cvxpnpl_amd_refine_robust.h); scale_px: finite and positive for
 * huber and cauchy, ignored by l2. */

/*
 * Batch form: the arguments of cvxpnpl_refine_vjp_batch, plus
 *   loss, scale_px               the loss the poses were refined under
 *   d_w_pts [batch][n_p], d_w_lines [batch][n_l]   the weights; either may be NULL (all 1)
 *   d_g_w_pts [batch][n_p], d_g_w_lines [batch][n_l]   the weights' gradients; either may be NULL (not wanted).  They may be asked for
 *                                with the weights absent: the derivative at w = 1.
 * 16 lanes per problem, one launch.  Asynchronous on `stream`.  Returns 0, -1 bad arguments (nothing is launched), -2 HIP error.
 * batch = 0 is a no-op.
 */
int cvxpnpl_refine_robust_vjp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l,
                                    const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R,
                                    const double *d_t, const int32_t *d_refine_status, int64_t status_stride, uint32_t admit_mask, int32_t loss,
                                    double scale_px, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_w_pts,
                                    const double *d_w_lines, const double *d_grad_R, const double *d_grad_t, double *d_g_pts_2d, double *d_g_pts_3d,
                                    double *d_g_line_2d, double *d_g_line_3d, double *d_g_w_pts, double *d_g_w_lines, int32_t *d_vjp_status,
                                    double *d_info, void *stream);

/* The same on the host: HOST pointers, n_threads host threads (<= 0: all cores) instead of a stream; the same source
 * (refine_robust_vjp_core.h) as the kernels.  Returns 0, or -1 for bad arguments. */
int cvxpnpl_refine_robust_vjp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                         const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                         const int32_t *refine_status, int64_t status_stride, uint32_t admit_mask, int32_t loss, double scale_px,
                                         const uint8_t *mask_pts, const uint8_t *mask_lines, const double *w_pts, const double *w_lines,
                                         const double *grad_R, const double *grad_t, double *g_pts_2d, double *g_pts_3d, double *g_line_2d,
                                         double *g_line_3d, double *g_w_pts, double *g_w_lines, int32_t *vjp_status, double *info, int32_t n_threads);

/*
 * Packed scenes, the layout of cvxpnpl_refine_vjp_scenes; d_w_pts [n_pts], d_w_lines [n_lines] and their gradients d_g_w_pts [n_pts],
 * d_g_w_lines [n_lines] in the packed layouts.  A scene writes the records of its own slices.  One workgroup per scene, one launch.
 * n_scenes = 0 is a no-op.
 */
int cvxpnpl_refine_robust_vjp_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                     const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                     const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_refine_status,
                                     int64_t status_stride, uint32_t admit_mask, int32_t loss, double scale_px, const uint8_t *d_mask_pts,
                                     const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, const double *d_grad_R,
                                     const double *d_grad_t, double *d_g_pts_2d, double *d_g_pts_3d, double *d_g_line_2d, double *d_g_line_3d,
                                     double *d_g_w_pts, double *d_g_w_lines, int32_t *d_vjp_status, double *d_info, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_refine_robust_grad_last_error(void);

const char *cvxpnpl_refine_robust_grad_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_REFINE_ROBUST_GRAD_H */
