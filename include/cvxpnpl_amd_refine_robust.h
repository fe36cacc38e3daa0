/*
 * cvxpnpl_amd_refine_robust.h -- C ABI of the reprojection refinement under a robust loss and per-correspondence weights
 * (libcvxpnpl_amd_refine_robust.so).
 *
 * The seventh library.  None of the other six depends on it and it depends on none of them; its kernels are held against a resource table
 * of their own (tests/golden/refine_robust_kernel_resources.json).  Conventions of the other ABIs: plain pointers and sizes, contiguous
 * float64 arrays, DEVICE pointers on the current device unless stated otherwise.
 *
 * What it computes.  The residuals, the chart, the Levenberg-Marquardt schedule and the statuses are those of
 * cvxpnpl_amd_refine.h.  The objective is
 *     f = sum_k w_k rho(s_k),     s_k = the sum of the two squared residuals of correspondence k
 * (a point: its squared pixel distance; a line: the two squared end-point distances), w_k the caller's weight (1 when the pointer is
 * NULL), and with delta = scale_px
 *     loss 0  l2       rho(s) = s
 *     loss 1  huber    rho(s) = s for s <= delta^2, 2 delta sqrt(s) - delta^2 above
 *     loss 2  cauchy   rho(s) = delta^2 log1p(s / delta^2).
 * The normal equations are re-weighted by omega_k = w_k rho'(s_k) at the pose reached (the rho'' term is dropped); the weights are
 * evaluated again at every pose, there is no inner loop; trials are judged by f.
 * LIVE: mask byte absent or non-zero, for a line a != b, and w_k != 0.  A zero weight is a mask: the record is not read and does not count
 * in n_live.  A weight that is negative or not finite, in a record that its mask admits, gives status CVXPNPL_REFINE_BEHIND (4) -- checked
 * after the causes of status 2 and before the count of live records.
 */
#ifndef CVXPNPL_AMD_REFINE_ROBUST_H
#define CVXPNPL_AMD_REFINE_ROBUST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CVXPNPL_LOSS_L2 = 0, CVXPNPL_LOSS_HUBER = 1, CVXPNPL_LOSS_CAUCHY = 2 };

/* Options; NULL means the defaults.  struct_size must be sizeof(cvxpnpl_refine_robust_opts_t). */
typedef struct {
    uint32_t struct_size;
    int32_t max_iters; /* 30 */
    double step_tol;   /* 1e-10 */
    double lambda0;    /* 1e-3 */
    int32_t loss;      /* CVXPNPL_LOSS_HUBER */
    double scale_px;   /* 1.0; finite and > 0 for huber and cauchy, ignored for l2 */
} cvxpnpl_refine_robust_opts_t;

/*
 * Batch form: the arguments of cvxpnpl_refine_batch, and
 *   d_w_pts [batch][n_p], d_w_lines [batch][n_l]   optional weights
 * outputs: d_R_out, d_t_out (may alias the inputs), d_cost [batch][2] (f before and after), d_iters, d_status_out, d_n_live [batch] int32
 *   as there (statuses 0-4; for 2-4 the pose passes through bit for bit, the costs are NaN, iters is 0; a pose that no trial has moved
 *   passes through bit for bit as well), and
 *   d_robust_w [batch][n_p + n_l]   optional: rho'(s_k) at the returned pose for every record, points then lines; 0 for a record that is
 *                                   not live, NaN for every record of a problem with status 2-4
 *   d_n_inlier [batch] int32        live records with s_k <= delta^2 at the returned pose (n_live for l2; 0 for status 2-4)
 * 16 lanes per problem, the whole loop in one launch, the per-record outputs in a second one.  Asynchronous on `stream`.
 * Returns 0, -1 bad arguments (nothing launched), -2 HIP error.  batch = 0 is a no-op whatever the pointers.
 */
int cvxpnpl_refine_robust_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines,
                                const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w, int32_t *d_n_inlier, void *stream);

/* The same on the host: HOST pointers, n_threads host threads (<= 0: all cores) instead of a stream; the same source
 * (refine_robust_core.h) as the kernels.  Returns 0, or -1 for bad arguments. */
int cvxpnpl_refine_robust_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                     const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                     const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                     const uint8_t *mask_lines, const double *w_pts, const double *w_lines,
                                     const cvxpnpl_refine_robust_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters,
                                     int32_t *status_out, int32_t *n_live, double *robust_w, int32_t *n_inlier, int32_t n_threads);

/*
 * Packed scenes: the arguments of cvxpnpl_refine_scenes, d_w_pts [n_pts] / d_w_lines [n_lines] optional weights, and the per-record
 * output in the packed layout: d_robust_w_pts [n_pts], d_robust_w_lines [n_lines] (each optional; only the records inside some scene's
 * slice are written).  One workgroup per scene.
 */
int cvxpnpl_refine_robust_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                 const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                 const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status,
                                 int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                                 const double *d_w_pts, const double *d_w_lines, const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out,
                                 double *d_t_out, double *d_cost, int32_t *d_iters, int32_t *d_status_out, int32_t *d_n_live,
                                 double *d_robust_w_pts, double *d_robust_w_lines, int32_t *d_n_inlier, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_refine_robust_last_error(void);

const char *cvxpnpl_refine_robust_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_REFINE_ROBUST_H */
