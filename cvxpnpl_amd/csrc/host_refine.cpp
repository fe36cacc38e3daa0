// host_refine.cpp -- host entry point of the reprojection refinement (cvxpnpl_refine_batch_host): a threaded loop over the same core
// (refine_core.h) as the device kernels (refine_kernel.h), so that the CPU test suite reaches the same mathematics.  The argument
// contract and the error text are refine_entry.h's; check_common holds what is this library's own, for the device entry points
// (refine_hip.hip, linked into the same library) too.
#include "../../include/cvxpnpl_amd_refine.h"
#include "refine_entry.h"

namespace cvxr {

// K and the poses, the outputs, the status column, the options: what the three entry points check once the sizes are known to be positive
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t,
                                                       const int32_t *status, int64_t status_stride, const cvxpnpl_refine_opts_t *opts, const void *R_out,
                                                       const void *t_out, const void *cost, const void *iters, const void *status_out, const void *n_live,
                                                       Opts &o)
{
    if (const char *m = cvxre::check_pose(K_per, K, R, t)) return cvxre::bad_args(who, m);
    if (!R_out || !t_out || !cost || !iters || !status_out || !n_live) return cvxre::bad_args(who, "an output pointer other than cov is null");
    if (const char *m = cvxre::check_status(status, status_stride)) return cvxre::bad_args(who, m);
    if (const char *m = cvxre::check_lm_opts(opts, "opts->struct_size is not sizeof(cvxpnpl_refine_opts_t)", o)) return cvxre::bad_args(who, m);
    if (opts) {
        if (!(opts->sigma_px >= 0.0) || !std::isfinite(opts->sigma_px)) return cvxre::bad_args(who, "sigma_px is not a finite non-negative number");
        o.sigma_px = opts->sigma_px;
    }
    return 0;
}

} // namespace cvxr

extern "C" const char *cvxpnpl_refine_last_error(void) { return cvxre::err_buf(); }

extern "C" const char *cvxpnpl_refine_version(void) { return "cvxpnpl_amd_refine 1"; }

extern "C" int cvxpnpl_refine_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                         const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                         const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                         const uint8_t *mask_lines, const cvxpnpl_refine_opts_t *opts, double *R_out, double *t_out, double *cost,
                                         int32_t *iters, int32_t *status_out, int32_t *n_live, double *cov, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    cvxr::Opts o;
    if (int rc = cvxr::check_common(who, K_per_problem, K, R, t, status, status_stride, opts, R_out, t_out, cost, iters, status_out, n_live, o)) return rc;
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxr::HostLanes ln;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, status, status_stride,
                                                   admit_mask, mask_pts, mask_lines, ln.pb, admit);
            cvxr::Result res;
            cvxr::refine_problem(ln, Kb, R + 9 * b, t + 3 * b, admit, o, res, cost + 2 * b);
            const bool done = res.status <= cvxr::REFINE_MAXITER; // otherwise the input pose passes through bit for bit
            for (int i = 0; i < 9; ++i) R_out[9 * b + i] = done ? res.R[i] : R[9 * b + i];
            for (int i = 0; i < 3; ++i) t_out[3 * b + i] = done ? res.t[i] : t[3 * b + i];
            cost[2 * b + 1] = res.cost;
            iters[b] = res.iters; status_out[b] = res.status; n_live[b] = res.n_live;
            if (cov) cvxr::covariance_problem(ln, Kb, R_out + 9 * b, t_out + 3 * b, res.status, res.cost, res.n_live, o, cov + 36 * b);
        }
    });
    return 0;
}
