// host_refine_robust.cpp -- host entry point of the robust reprojection refinement (cvxpnpl_refine_robust_batch_host): a threaded loop over
// the same core (refine_robust_core.h) as the device kernels (refine_robust_kernel.h), so that the CPU test suite reaches the same
// mathematics.  The argument contract and the error text are refine_entry.h's; check_common holds what is this library's own, for the
// device entry points (refine_robust_hip.hip, linked into the same library) too.
#include "../../include/cvxpnpl_amd_refine_robust.h"
#include "refine_entry.h"
#include "refine_robust_core.h"

namespace cvxrb {

// K and the poses, the outputs, the status column, the options: what the three entry points check once the sizes are known to be positive
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                       int64_t status_stride, const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out,
                                                       const void *cost, const void *iters, const void *status_out, const void *n_live,
                                                       const void *n_inlier, Opts &o, int &loss, double &scale_px)
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

} // namespace cvxrb

extern "C" const char *cvxpnpl_refine_robust_last_error(void) { return cvxre::err_buf(); }

extern "C" const char *cvxpnpl_refine_robust_version(void) { return "cvxpnpl_amd_refine_robust 1"; }

extern "C" int cvxpnpl_refine_robust_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                                const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                                const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                                const uint8_t *mask_lines, const double *w_pts, const double *w_lines,
                                                const cvxpnpl_refine_robust_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters,
                                                int32_t *status_out, int32_t *n_live, double *robust_w, int32_t *n_inlier, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_robust_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    cvxrb::Opts o;
    int loss;
    double scale_px;
    if (int rc = cvxrb::check_common(who, K_per_problem, K, R, t, status, status_stride, opts, R_out, t_out, cost, iters, status_out, n_live, n_inlier, o, loss, scale_px))
        return rc;
    const cvxrb::Loss l = cvxrb::make_loss(loss, scale_px);
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxrb::HostLanes ln;
            cvxrb::WProb &wp = ln.wp;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, status, status_stride,
                                                   admit_mask, mask_pts, mask_lines, wp.pb, admit);
            cvxre::host_weights(wp, b, n_p, n_l, w_pts, w_lines);
            wp.ow_p = robust_w ? robust_w + b * ((int64_t)n_p + n_l) : nullptr;
            wp.ow_l = wp.ow_p ? wp.ow_p + n_p : nullptr;
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
