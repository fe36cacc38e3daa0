/*
 * cvxpnpl_amd_refine.h -- C ABI of the reprojection refinement of poses (libcvxpnpl_amd_refine.so).
 *
 * The fifth library, beside the solver's, the backward pass's and the two RANSAC libraries: none of them depends on it, and its kernels
 * are held against a resource table of their own (tests/golden/refine_kernel_resources.json).  Same conventions as the other ABIs: plain
 * pointers and sizes, contiguous float64 arrays, DEVICE pointers on the current device unless stated otherwise.
 *
 * What it computes.  Given a pose (R, t) per problem, a few Levenberg-Marquardt iterations on PIXEL residuals:
 *   a point (x, y) <-> X gives pi(K (R X + t)) - (x, y); a line (a, b) <-> (E0, E1) gives, for both end points, the signed distance of the
 *   projected end point from the image line through a and b.  The cost is the sum of squares over LIVE correspondences: mask byte absent
 *   or non-zero, and for a line a != b.  Correspondences that are not live never enter the arithmetic.
 * Schedule: lambda_0 = lambda0; (J^T J + lambda diag(J^T J)) d = -J^T r by Cholesky; a trial is accepted iff every live record keeps
 * depth > 0 and the cost does not increase; accept: lambda / 10 (at least 1e-12), reject: 10 lambda, beyond 1e12 the run ends.  CONVERGED
 * is an accepted step with |d| <= step_tol (1 + |t|) -- or a rejected trial at lambda <= lambda0 that is that small or costs no more than
 * 1e-12 of the cost above it: the pose has reached the rounding floor of the cost, where the comparison of the two costs is chance.
 * Every trial counts in max_iters.  All arithmetic float64.
 * The chart of the covariance is xi = (w, tau): R' = exp([w]x) R, t' = t + tau, so that cov[3:,3:] is the covariance of t.
 */
#ifndef CVXPNPL_AMD_REFINE_H
#define CVXPNPL_AMD_REFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CVXPNPL_REFINE_CONVERGED = 0,
    CVXPNPL_REFINE_MAXITER = 1,  /* max_iters trials, or lambda beyond 1e12: the cost has not increased, the pose is the best accepted */
    CVXPNPL_REFINE_SKIPPED = 2,  /* input status not in admit_mask, a non-finite pose, or det R <= 0 (a reflection cannot be repaired) */
    CVXPNPL_REFINE_SINGULAR = 3, /* fewer than 3 live correspondences, or no lambda gave a positive definite system */
    CVXPNPL_REFINE_BEHIND = 4    /* a live record has depth <= 0 at the input pose, or holds a number that is not finite (NaN or inf in its
                                    2D or its 3D half: the cost at the input pose is not a number) */
};
/* For statuses 2-4 the output pose is the input pose bit for bit, cost and covariance are NaN, iters is 0.  With status 0 or 1 a pose that
 * no trial has moved (max_iters = 0, or converged on a rejected trial) is the input pose bit for bit as well. */

/* Options; NULL means the defaults.  struct_size must be sizeof(cvxpnpl_refine_opts_t): a caller built against another layout is refused. */
typedef struct {
    uint32_t struct_size;
    int32_t max_iters; /* 30 */
    double step_tol;   /* 1e-10 */
    double lambda0;    /* 1e-3 */
    double sigma_px;   /* 0: the covariance is scaled by cost_after / (m - 6), m = 2 * live correspondences; > 0: by sigma_px^2 */
} cvxpnpl_refine_opts_t;

/*
 * Batch form: the layouts of cvxpnpl_solve_batch (d_pts_2d [batch][n_p][2], d_pts_3d [batch][n_p][3], d_line_2d [batch][n_l][2][2],
 * d_line_3d [batch][n_l][2][3], d_K [3][3] or [batch][3][3]) and poses d_R [batch][9], d_t [batch][3].
 *   d_status, status_stride   optional input statuses, problem b reads d_status[b * status_stride] (a column of a wider table can be
 *                             passed as it is); admit_mask: bit s set = status s is refined (0x5: CERTIFIED and UNCERTIFIED)
 *   d_mask_pts [batch][n_p], d_mask_lines [batch][n_l]   optional uint8, non-zero = live
 * outputs: d_R_out [batch][9], d_t_out [batch][3] (may alias the inputs), d_cost [batch][2] (sum of squared pixel residuals before and
 *   after), d_iters, d_status_out, d_n_live [batch] int32, d_cov [batch][36] (optional): sigma^2 (J^T J)^-1 at the final pose, Gauss-Newton
 *   J, no damping, public chart; NaN when m <= 6 without sigma_px or when J^T J is not positive definite.
 * 16 lanes per problem, the whole loop in one launch.  Asynchronous on `stream`.  Returns 0, -1 bad arguments, -2 HIP error.
 */
int cvxpnpl_refine_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                         const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                         const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                         const cvxpnpl_refine_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                         int32_t *d_status_out, int32_t *d_n_live, double *d_cov, void *stream);

/* The same on the host: HOST pointers, n_threads host threads (<= 0: all cores) instead of a stream; the same source (refine_core.h) as
 * the kernels.  Returns 0, or -1 for bad arguments. */
int cvxpnpl_refine_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                              const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                              const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts, const uint8_t *mask_lines,
                              const cvxpnpl_refine_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters, int32_t *status_out,
                              int32_t *n_live, double *cov, int32_t n_threads);

/*
 * Packed scenes, the layout of the RANSAC libraries: scene f is the points d_pt_offsets[f] .. d_pt_offsets[f+1] of d_pts_2d [n_pts][2] /
 * d_pts_3d [n_pts][3] and the lines d_ln_offsets[f] .. d_ln_offsets[f+1] of d_line_2d [n_lines][2][2] / d_line_3d [n_lines][2][3]
 * (d_ln_offsets may be NULL when n_lines is 0); offsets are clamped to the packed arrays.  d_K [3][3] or [n_scenes][3][3]; one pose per
 * scene; d_mask_pts [n_pts], d_mask_lines [n_lines] optional.  The other arguments and the outputs are those of cvxpnpl_refine_batch with
 * n_scenes for batch.  One workgroup per scene, the whole loop in one launch.
 */
int cvxpnpl_refine_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                          const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                          int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status, int64_t status_stride,
                          uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const cvxpnpl_refine_opts_t *opts,
                          double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters, int32_t *d_status_out, int32_t *d_n_live, double *d_cov,
                          void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_refine_last_error(void);

const char *cvxpnpl_refine_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_REFINE_H */
