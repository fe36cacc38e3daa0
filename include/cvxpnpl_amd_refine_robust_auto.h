/*
 * cvxpnpl_amd_refine_robust_auto.h -- C ABI of the robust refinement with a scale per problem: a scale estimate from the median squared
 * residual, the loop of cvxpnpl_amd_refine_robust.h at one scale per problem, and the sandwich covariance of the robust minimum
 * (libcvxpnpl_amd_refine_robust_auto.so).
 *
 * The twelfth library.  None of the other eleven depends on it and it depends on none of them; its kernels are held against a resource
 * table of their own (tests/golden/refine_robust_auto_kernel_resources.json).  Conventions of the other ABIs: plain pointers and sizes,
 * contiguous float64 arrays, DEVICE pointers on the current device unless stated otherwise.  The residuals, s_k, the losses, LIVE, the
 * statuses and the options struct are those of cvxpnpl_amd_refine_robust.h (included below); DESIGN.md section 22 has the definitions.
 *
 * Every function returns 0, -1 for bad arguments (nothing launched) or -2 for a HIP error; a zero batch / scene count is a no-op whatever
 * the pointers; the device forms are asynchronous on `stream`; the host forms take HOST pointers and n_threads (<= 0: all cores) and run
 * the same source as the kernels.
 */
#ifndef CVXPNPL_AMD_REFINE_ROBUST_AUTO_H
#define CVXPNPL_AMD_REFINE_ROBUST_AUTO_H

#include <stddef.h>
#include <stdint.h>

#include "cvxpnpl_amd_refine_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * 1. The scale of every problem at its pose (R, t).  With s_(0) <= ... <= s_(m-1) the s_k of the m live records,
 *      med_sq = s_((m-1)/2) for odd m, 0.5 (s_(m/2-1) + s_(m/2)) for even m          (numpy.median)
 *      sigma  = sqrt(med_sq / 1.3862943611198906)                                    (2 ln 2, the median of chi^2 with 2 degrees)
 * The median is UNWEIGHTED: a weight decides whether a record is live (w != 0) and nothing else.  That is a decision: a weighted median
 * would make the scale depend on the matcher's confidences, which are not noise levels.  The order statistics are found exactly (a walk
 * over the bit pattern, no sort, no atomics), so med_sq is made of elements of sq bit for bit.
 * The arguments up to the weights are those of cvxpnpl_refine_robust_batch / _scenes / _batch_host.  Outputs, all required:
 *   d_sigma, d_med_sq [n] f64      NaN for statuses 2-4
 *   d_n_live, d_status_out [n] i32 the entry checks of the refinement in its order: 2 not admitted, non-finite pose or det R <= 0; 4 a bad
 *                                  weight; 3 fewer than 3 live records; 4 a live record behind the camera or with a non-finite s; else 0
 *   d_sq                           s_k per record and the selection's workspace: batch form [n][n_p + n_l], points then lines; scenes
 *                                  form the packed pair [n_pts], [n_lines] (only records inside some scene's slice are written).
 *                                  s_k of a live record, exactly -1.0 for a record that is not live, NaN for every record of a problem
 *                                  with status 2-4.
 */
int cvxpnpl_robust_scale_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                               const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                               const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                               const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, double *d_sigma, double *d_med_sq,
                               int32_t *d_n_live, int32_t *d_status_out, double *d_sq, void *stream);

int cvxpnpl_robust_scale_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                    const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                    const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                    const uint8_t *mask_lines, const double *w_pts, const double *w_lines, double *sigma, double *med_sq,
                                    int32_t *n_live, int32_t *status_out, double *sq, int32_t n_threads);

int cvxpnpl_robust_scale_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                                int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status, int64_t status_stride,
                                uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_w_pts,
                                const double *d_w_lines, double *d_sigma, double *d_med_sq, int32_t *d_n_live, int32_t *d_status_out,
                                double *d_sq_pts, double *d_sq_lines, void *stream);

/*
 * 2. cvxpnpl_refine_robust_batch / _batch_host / _scenes with one more argument after the weights:
 *   d_scale_px [batch] / [n_scenes]   the scale of every problem; NULL: opts->scale_px for all, and the result is that library's bit for bit.
 * Under l2 the array is not read.  Under huber and cauchy an element that is not finite and > 0 gives its problem status 4 at the place
 * where a bad weight does (after the causes of status 2, before the count of live records), and the pose passes through; opts->scale_px
 * is then only checked as that library checks it.  robust_w and n_inlier are taken at the problem's own scale.
 */
int cvxpnpl_refine_robust_pp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                   const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                   const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                   const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, const double *d_scale_px,
                                   const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                   int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w, int32_t *d_n_inlier, void *stream);

int cvxpnpl_refine_robust_pp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                        const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                        const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                        const uint8_t *mask_lines, const double *w_pts, const double *w_lines, const double *scale_px,
                                        const cvxpnpl_refine_robust_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters,
                                        int32_t *status_out, int32_t *n_live, double *robust_w, int32_t *n_inlier, int32_t n_threads);

int cvxpnpl_refine_robust_pp_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                    const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                    const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status,
                                    int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                                    const double *d_w_pts, const double *d_w_lines, const double *d_scale_px,
                                    const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                    int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w_pts, double *d_robust_w_lines,
                                    int32_t *d_n_inlier, void *stream);

/*
 * 3. The sandwich covariance of a robustly refined pose.  In the chart about the mean of the live 3D records, with v_k = sum_i J_i r_i
 * over the two residuals of record k and omega_k = w_k rho'(s_k),
 *      H = the full Hessian of 1/2 sum w rho (residual curvature and the 2 w rho'' v v^T term, cvxpnpl_amd_refine_robust_grad.h's),
 *      B = sum_k omega_k^2 v_k v_k^T,        V_c = m / (m - 6) H^-1 B H^-1,      m = 2 n_live,
 * brought to the public chart xi = (w, tau) of cvxpnpl_amd_refine.h: cov = M V_c M^T, cov[3:,3:] the covariance of t.
 * Inputs: the correspondences, masks and weights as above; the pose; d_status [n] (optional, unit stride), the refinement's status of the
 * pose: only 0 and 1 are differentiated; the loss (CVXPNPL_LOSS_*) and its scale, scale_px for all or d_scale_px [n] when not NULL (l2
 * reads neither).  Outputs, both required:
 *   d_cov [n][36]          NaN unless the status is 0
 *   d_cov_status [n] i32   0 ok; 2 not differentiated (or a non-finite pose, det R <= 0); 3 m <= 6, or H is not positive definite: the
 *                          pose is not a strict minimum; 4 a bad weight or scale element, a live record behind the camera or non-finite
 */
int cvxpnpl_robust_cov_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                             const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                             const int32_t *d_status, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_w_pts,
                             const double *d_w_lines, int32_t loss, double scale_px, const double *d_scale_px, double *d_cov, int32_t *d_cov_status,
                             void *stream);

int cvxpnpl_robust_cov_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                  const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                  const int32_t *status, const uint8_t *mask_pts, const uint8_t *mask_lines, const double *w_pts,
                                  const double *w_lines, int32_t loss, double scale_px, const double *scale_px_each, double *cov, int32_t *cov_status,
                                  int32_t n_threads);

int cvxpnpl_robust_cov_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                              const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                              int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status, const uint8_t *d_mask_pts,
                              const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, int32_t loss, double scale_px,
                              const double *d_scale_px, double *d_cov, int32_t *d_cov_status, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_refine_robust_auto_last_error(void);

const char *cvxpnpl_refine_robust_auto_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_REFINE_ROBUST_AUTO_H */
