// host_refine_robust.cpp -- host entry point of the robust reprojection refinement (cvxpnpl_refine_robust_batch_host): a threaded loop over
// the same core (refine_robust_core.h) as the device kernels (refine_robust_kernel.h), so that the CPU test suite reaches the same
// mathematics.  Also the argument checks and the error text that the device entry points (refine_robust_hip.hip, linked into the same
// library) share with it.
#include <algorithm>
#include <cmath>
#include <stdio.h>
#include <thread>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_robust.h"
#include "refine_robust_core.h"

namespace cvxrb {

// (hidden: the library exports what its header declares and nothing else; refine_robust_hip.hip declares the same three)
__attribute__((visibility("hidden"))) char *err_buf();
__attribute__((visibility("hidden"))) int bad_args(const char *who, const char *what);
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                       int64_t status_stride, const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out,
                                                       const void *cost, const void *iters, const void *status_out, const void *n_live,
                                                       const void *n_inlier, Opts &o, int &loss, double &scale_px);

char *err_buf()
{
    static thread_local char buf[512] = "";
    return buf;
}

int bad_args(const char *who, const char *what)
{
    snprintf(err_buf(), 512, "%s: bad arguments (%s)", who, what);
    return -1;
}

// what the three entry points share once the sizes are known to be positive: K, the poses, the options, the outputs
int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status, int64_t status_stride,
                 const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out, const void *cost, const void *iters,
                 const void *status_out, const void *n_live, const void *n_inlier, Opts &o, int &loss, double &scale_px)
{
    if (K_per != 0 && K_per != 1) return bad_args(who, "K_per_problem / K_per_scene is 0 or 1");
    if (!K || !R || !t) return bad_args(who, "K, R or t is null");
    if (!R_out || !t_out || !cost || !iters || !status_out || !n_live || !n_inlier) return bad_args(who, "an output pointer other than robust_w is null");
    if (status && status_stride < 0) return bad_args(who, "negative status_stride");
    o.max_iters = 30; o.step_tol = 1e-10; o.lambda0 = 1e-3; o.sigma_px = 0.0;
    loss = CVXPNPL_LOSS_HUBER;
    scale_px = 1.0;
    if (opts) {
        if (opts->struct_size != sizeof(cvxpnpl_refine_robust_opts_t)) return bad_args(who, "opts->struct_size is not sizeof(cvxpnpl_refine_robust_opts_t)");
        if (opts->max_iters < 0) return bad_args(who, "negative max_iters");
        if (!(opts->step_tol >= 0.0) || !std::isfinite(opts->step_tol)) return bad_args(who, "step_tol is not a finite non-negative number");
        if (!(opts->lambda0 >= 0.0) || !std::isfinite(opts->lambda0)) return bad_args(who, "lambda0 is not a finite non-negative number");
        if (opts->loss < CVXPNPL_LOSS_L2 || opts->loss > CVXPNPL_LOSS_CAUCHY) return bad_args(who, "loss is 0 (l2), 1 (huber) or 2 (cauchy)");
        if (opts->loss != CVXPNPL_LOSS_L2 && (!(opts->scale_px > 0.0) || !std::isfinite(opts->scale_px)))
            return bad_args(who, "scale_px is not a finite positive number");
        o.max_iters = opts->max_iters; o.step_tol = opts->step_tol; o.lambda0 = opts->lambda0;
        loss = opts->loss; scale_px = opts->scale_px;
    }
    return 0;
}

} // namespace cvxrb

extern "C" const char *cvxpnpl_refine_robust_last_error(void) { return cvxrb::err_buf(); }

extern "C" const char *cvxpnpl_refine_robust_version(void) { return "cvxpnpl_amd_refine_robust 1"; }

extern "C" int cvxpnpl_refine_robust_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                                const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                                const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                                const uint8_t *mask_lines, const double *w_pts, const double *w_lines,
                                                const cvxpnpl_refine_robust_opts_t *opts, double *R_out, double *t_out, double *cost, int32_t *iters,
                                                int32_t *status_out, int32_t *n_live, double *robust_w, int32_t *n_inlier, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_robust_batch_host";
    if (batch < 0 || n_p < 0 || n_l < 0 || (int64_t)n_p + n_l > 0x7fffffffLL) return cvxrb::bad_args(who, "negative size");
    if (batch == 0) return 0;
    if ((n_p > 0 && (!pts_2d || !pts_3d)) || (n_l > 0 && (!line_2d || !line_3d))) return cvxrb::bad_args(who, "a correspondence pointer is null");
    cvxrb::Opts o;
    int loss;
    double scale_px;
    if (int rc = cvxrb::check_common(who, K_per_problem, K, R, t, status, status_stride, opts, R_out, t_out, cost, iters, status_out, n_live, n_inlier, o, loss, scale_px))
        return rc;
    const cvxrb::Loss l = cvxrb::make_loss(loss, scale_px);
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > batch) nt = (int)batch;
    auto work = [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            const cvx::ProblemView pv = cvx::make_view(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem);
            cvxrb::HostLanes ln;
            cvxrb::WProb &wp = ln.wp;
            wp.pb.n_p = n_p; wp.pb.n_l = n_l;
            wp.pb.p2 = pv.p2; wp.pb.p3 = pv.p3; wp.pb.l2 = pv.l2; wp.pb.l3 = pv.l3;
            wp.pb.mp = mask_pts && n_p > 0 ? mask_pts + b * n_p : nullptr;
            wp.pb.ml = mask_lines && n_l > 0 ? mask_lines + b * n_l : nullptr;
            wp.wp = w_pts && n_p > 0 ? w_pts + b * n_p : nullptr;
            wp.wl = w_lines && n_l > 0 ? w_lines + b * n_l : nullptr;
            wp.ow_p = robust_w ? robust_w + b * ((int64_t)n_p + n_l) : nullptr;
            wp.ow_l = wp.ow_p ? wp.ow_p + n_p : nullptr;
            const bool admit = !status || cvxr::admitted(status[b * status_stride], admit_mask);
            cvxrb::Result res;
            cvxrb::robust_problem(ln, pv.K, R + 9 * b, t + 3 * b, admit, o, l, res, cost[2 * b]);
            const bool done = res.status <= cvxr::REFINE_MAXITER; // otherwise the input pose passes through bit for bit
            for (int i = 0; i < 9; ++i) R_out[9 * b + i] = done ? res.R[i] : R[9 * b + i];
            for (int i = 0; i < 3; ++i) t_out[3 * b + i] = done ? res.t[i] : t[3 * b + i];
            cost[2 * b + 1] = res.cost;
            iters[b] = res.iters; status_out[b] = res.status; n_live[b] = res.n_live;
            n_inlier[b] = cvxrb::robust_weights_problem(ln, wp, pv.K, R_out + 9 * b, t_out + 3 * b, res.status, l);
        }
    };
    if (nt == 1) { work(0, batch); return 0; }
    std::vector<std::thread> pool;
    const int64_t chunk = (batch + nt - 1) / nt;
    for (int k = 0; k < nt; ++k) {
        const int64_t lo = k * chunk, hi = std::min<int64_t>(batch, lo + chunk);
        if (lo < hi) pool.emplace_back(work, lo, hi);
    }
    for (auto &th : pool) th.join();
    return 0;
}
