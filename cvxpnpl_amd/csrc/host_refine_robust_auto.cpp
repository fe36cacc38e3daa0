// host_refine_robust_auto.cpp -- host entry points of the twelfth library (cvxpnpl_robust_scale_batch_host,
// cvxpnpl_refine_robust_pp_batch_host, cvxpnpl_robust_cov_batch_host): threaded loops over the same cores (refine_robust_auto_core.h,
// refine_robust_core.h) as the device kernels (refine_robust_auto_kernel.h), so that the CPU test suite reaches the same mathematics.  The
// argument contract and the error text are refine_entry.h's; the check_* functions hold what is this library's own, for the device entry
// points (refine_robust_auto_hip.hip, linked into the same library) too.
#include "../../include/cvxpnpl_amd_refine_robust_auto.h"
#include "refine_entry.h"
#include "refine_robust_auto_core.h"

namespace cvxra {

// what the scale entry points check once the sizes are known to be positive: K and the poses, the outputs, the status column
__attribute__((visibility("hidden"))) int check_scale(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                      int64_t status_stride, const void *sigma, const void *med_sq, const void *n_live, const void *status_out,
                                                      bool sq_given)
{
    if (const char *m = cvxre::check_pose(K_per, K, R, t)) return cvxre::bad_args(who, m);
    if (!sigma || !med_sq || !n_live || !status_out || !sq_given) return cvxre::bad_args(who, "an output pointer is null (sq is the selection's workspace)");
    if (const char *m = cvxre::check_status(status, status_stride)) return cvxre::bad_args(who, m);
    return 0;
}

// ... the loop's: cvxpnpl_amd_refine_robust.h's checks (host_refine_robust.cpp's check_common)
__attribute__((visibility("hidden"))) int check_loop(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                     int64_t status_stride, const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out,
                                                     const void *cost, const void *iters, const void *status_out, const void *n_live, const void *n_inlier,
                                                     cvxr::Opts &o, int &loss, double &scale_px)
{
    if (const char *m = cvxre::check_pose(K_per, K, R, t)) return cvxre::bad_args(who, m);
    if (!R_out || !t_out || !cost || !iters || !status_out || !n_live || !n_inlier)
        return cvxre::bad_args(who, "an output pointer other than robust_w is null");
    if (const char *m = cvxre::check_status(status, status_stride)) return cvxre::bad_args(who, m);
    if (const char *m = cvxre::check_lm_opts(opts, "opts->struct_size is not sizeof(cvxpnpl_refine_robust_opts_t)", o)) return cvxre::bad_args(who, m);
    loss = opts ? opts->loss : CVXPNPL_LOSS_HUBER;
    scale_px = opts ? opts->scale_px : 1.0;
    if (const char *m = cvxre::check_loss(loss, scale_px)) return cvxre::bad_args(who, m);
    return 0;
}

// ... the covariance's (a uniform scale is checked only where it is the one in use)
__attribute__((visibility("hidden"))) int check_cov(const char *who, int32_t K_per, const double *K, const double *R, const double *t, int32_t loss, double scale_px,
                                                    const double *scale_each, const void *cov, const void *cov_status)
{
    if (const char *m = cvxre::check_pose(K_per, K, R, t)) return cvxre::bad_args(who, m);
    if (!cov || !cov_status) return cvxre::bad_args(who, "an output pointer is null");
    if (const char *m = cvxre::check_loss(loss, scale_each ? 1.0 : scale_px)) return cvxre::bad_args(who, m);
    return 0;
}

} // namespace cvxra

extern "C" const char *cvxpnpl_refine_robust_auto_last_error(void) { return cvxre::err_buf(); }

extern "C" const char *cvxpnpl_refine_robust_auto_version(void) { return "cvxpnpl_amd_refine_robust_auto 1"; }

extern "C" int cvxpnpl_robust_scale_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                               const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                               const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                               const uint8_t *mask_lines, const double *w_pts, const double *w_lines, double *sigma, double *med_sq,
                                               int32_t *n_live, int32_t *status_out, double *sq, int32_t n_threads)
{
    const char *who = "cvxpnpl_robust_scale_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_scale(who, K_per_problem, K, R, t, status, status_stride, sigma, med_sq, n_live, status_out, sq || n_p + n_l == 0)) return rc;
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxra::HostScaleLanes sl;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, status, status_stride,
                                                   admit_mask, mask_pts, mask_lines, sl.wp.pb, admit);
            cvxre::host_weights(sl.wp, b, n_p, n_l, w_pts, w_lines);
            sl.wp.ow_p = sq ? sq + b * ((int64_t)n_p + n_l) : nullptr;
            sl.wp.ow_l = sl.wp.ow_p ? sl.wp.ow_p + n_p : nullptr;
            cvxra::ScaleResult res;
            cvxra::scale_problem(sl, Kb, R + 9 * b, t + 3 * b, admit, res);
            sigma[b] = res.sigma; med_sq[b] = res.med_sq; n_live[b] = res.n_live; status_out[b] = res.status;
        }
    });
    return 0;
}

extern "C" int cvxpnpl_refine_robust_pp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                                   const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                                   const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                                   const uint8_t *mask_lines, const double *w_pts, const double *w_lines, const double *scale_each,
                                                   const cvxpnpl_refine_robust_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters,
                                                   int32_t *status_out, int32_t *n_live, double *robust_w, int32_t *n_inlier, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_robust_pp_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    cvxr::Opts o;
    int loss;
    double scale_px;
    if (int rc = cvxra::check_loop(who, K_per_problem, K, R, t, status, status_stride, opts, R_out, t_out, cost, iters, status_out, n_live, n_inlier, o, loss, scale_px))
        return rc;
    if (loss == CVXPNPL_LOSS_L2) scale_each = nullptr; // (not read)
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxra::PerProblemScale<cvxrb::HostLanes> ln;
            cvxrb::WProb &wp = ln.wp;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, status, status_stride,
                                                   admit_mask, mask_pts, mask_lines, wp.pb, admit);
            cvxre::host_weights(wp, b, n_p, n_l, w_pts, w_lines);
            wp.ow_p = robust_w ? robust_w + b * ((int64_t)n_p + n_l) : nullptr;
            wp.ow_l = wp.ow_p ? wp.ow_p + n_p : nullptr;
            const double scale = scale_each ? scale_each[b] : scale_px;
            ln.bad_scale = !cvxra::scale_usable(loss, scale);
            const cvxrb::Loss l = cvxrb::make_loss(loss, scale);
            cvxrb::Result res;
            cvxrb::robust_problem(ln, Kb, R + 9 * b, t + 3 * b, admit, o, l, res, cost[2 * b]);
            const bool done = res.status <= cvxr::REFINE_MAXITER; // otherwise the input pose passes through bit for bit
            for (int i = 0; i < 9; ++i) R_out[9 * b + i] = done ? res.R[i] : R[9 * b + i];
            for (int i = 0; i < 3; ++i) t_out[3 * b + i] = done ? res.t[i] : t[3 * b + i];
            cost[2 * b + 1] = res.cost;
            iters[b] = res.iters; status_out[b] = res.status; n_live[b] = res.n_live;
            n_inlier[b] = cvxrb::robust_weights_problem(ln, wp, Kb, R_out + 9 * b, t_out + 3 * b, res.status, l);
        }
    });
    return 0;
}

extern "C" int cvxpnpl_robust_cov_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                             const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                             const int32_t *status, const uint8_t *mask_pts, const uint8_t *mask_lines, const double *w_pts,
                                             const double *w_lines, int32_t loss, double scale_px, const double *scale_each, double *cov, int32_t *cov_status,
                                             int32_t n_threads)
{
    const char *who = "cvxpnpl_robust_cov_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_cov(who, K_per_problem, K, R, t, loss, scale_px, scale_each, cov, cov_status)) return rc;
    if (loss == CVXPNPL_LOSS_L2) scale_each = nullptr;
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxrb::HostLanes ln;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, nullptr, 1, 0u, mask_pts, mask_lines,
                                                   ln.wp.pb, admit);
            cvxre::host_weights(ln.wp, b, n_p, n_l, w_pts, w_lines);
            ln.wp.ow_p = ln.wp.ow_l = nullptr;
            const double scale = scale_each ? scale_each[b] : scale_px;
            const bool usable = cvxra::scale_usable(loss, scale);
            const bool diff = !status || status[b] == cvxr::REFINE_CONVERGED || status[b] == cvxr::REFINE_MAXITER;
            cov_status[b] = cvxra::robust_cov_problem(ln, Kb, R + 9 * b, t + 3 * b, diff, !usable, cvxrb::make_loss(loss, usable ? scale : 1.0), cov + 36 * b);
        }
    });
    return 0;
}
