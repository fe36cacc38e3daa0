// host_refine.cpp -- host entry point of the reprojection refinement (cvxpnpl_refine_batch_host): a threaded loop over the same core
// (refine_core.h) as the device kernels (refine_kernel.h), so that the CPU test suite reaches the same mathematics.  Also the argument
// checks and the error text that the device entry points (refine_hip.hip, linked into the same library) share with it.
#include <algorithm>
#include <cmath>
#include <stdio.h>
#include <thread>
#include <vector>

#include "../../include/cvxpnpl_amd_refine.h"
#include "refine_core.h"

namespace cvxr {

// (hidden: the library exports what its header declares and nothing else; refine_hip.hip declares the same three)
__attribute__((visibility("hidden"))) char *err_buf();
__attribute__((visibility("hidden"))) int bad_args(const char *who, const char *what);
__attribute__((visibility("hidden"))) int check_common(const char *who, int64_t n, int32_t K_per, const double *K, const double *R, const double *t,
                                                       const int32_t *status, int64_t status_stride, const cvxpnpl_refine_opts_t *opts, const void *R_out,
                                                       const void *t_out, const void *cost, const void *iters, const void *status_out, const void *n_live,
                                                       Opts &o);

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
int check_common(const char *who, int64_t n, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status, int64_t status_stride,
                 const cvxpnpl_refine_opts_t *opts, const void *R_out, const void *t_out, const void *cost, const void *iters, const void *status_out,
                 const void *n_live, Opts &o)
{
    (void)n;
    if (K_per != 0 && K_per != 1) return bad_args(who, "K_per_problem / K_per_scene is 0 or 1");
    if (!K || !R || !t) return bad_args(who, "K, R or t is null");
    if (!R_out || !t_out || !cost || !iters || !status_out || !n_live) return bad_args(who, "an output pointer other than cov is null");
    if (status && status_stride < 0) return bad_args(who, "negative status_stride");
    o.max_iters = 30; o.step_tol = 1e-10; o.lambda0 = 1e-3; o.sigma_px = 0.0;
    if (opts) {
        if (opts->struct_size != sizeof(cvxpnpl_refine_opts_t)) return bad_args(who, "opts->struct_size is not sizeof(cvxpnpl_refine_opts_t)");
        if (opts->max_iters < 0) return bad_args(who, "negative max_iters");
        if (!(opts->step_tol >= 0.0) || !std::isfinite(opts->step_tol)) return bad_args(who, "step_tol is not a finite non-negative number");
        if (!(opts->lambda0 >= 0.0) || !std::isfinite(opts->lambda0)) return bad_args(who, "lambda0 is not a finite non-negative number");
        if (!(opts->sigma_px >= 0.0) || !std::isfinite(opts->sigma_px)) return bad_args(who, "sigma_px is not a finite non-negative number");
        o.max_iters = opts->max_iters; o.step_tol = opts->step_tol; o.lambda0 = opts->lambda0; o.sigma_px = opts->sigma_px;
    }
    return 0;
}

} // namespace cvxr

extern "C" const char *cvxpnpl_refine_last_error(void) { return cvxr::err_buf(); }

extern "C" const char *cvxpnpl_refine_version(void) { return "cvxpnpl_amd_refine 1"; }

extern "C" int cvxpnpl_refine_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                         const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                         const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                         const uint8_t *mask_lines, const cvxpnpl_refine_opts_t *opts, double *R_out, double *t_out, double *cost,
                                         int32_t *iters, int32_t *status_out, int32_t *n_live, double *cov, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_batch_host";
    if (batch < 0 || n_p < 0 || n_l < 0 || (int64_t)n_p + n_l > 0x7fffffffLL) return cvxr::bad_args(who, "negative size");
    if (batch == 0) return 0;
    if ((n_p > 0 && (!pts_2d || !pts_3d)) || (n_l > 0 && (!line_2d || !line_3d))) return cvxr::bad_args(who, "a correspondence pointer is null");
    cvxr::Opts o;
    if (int rc = cvxr::check_common(who, batch, K_per_problem, K, R, t, status, status_stride, opts, R_out, t_out, cost, iters, status_out, n_live, o)) return rc;
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > batch) nt = (int)batch;
    auto work = [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            const cvx::ProblemView pv = cvx::make_view(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem);
            cvxr::HostLanes ln;
            ln.pb.n_p = n_p; ln.pb.n_l = n_l;
            ln.pb.p2 = pv.p2; ln.pb.p3 = pv.p3; ln.pb.l2 = pv.l2; ln.pb.l3 = pv.l3;
            ln.pb.mp = mask_pts ? mask_pts + b * n_p : nullptr;
            ln.pb.ml = mask_lines ? mask_lines + b * n_l : nullptr;
            const bool admit = !status || cvxr::admitted(status[b * status_stride], admit_mask);
            cvxr::Result res;
            cvxr::refine_problem(ln, pv.K, R + 9 * b, t + 3 * b, admit, o, res, cost + 2 * b);
            const bool done = res.status <= cvxr::REFINE_MAXITER; // otherwise the input pose passes through bit for bit
            for (int i = 0; i < 9; ++i) R_out[9 * b + i] = done ? res.R[i] : R[9 * b + i];
            for (int i = 0; i < 3; ++i) t_out[3 * b + i] = done ? res.t[i] : t[3 * b + i];
            cost[2 * b + 1] = res.cost;
            iters[b] = res.iters; status_out[b] = res.status; n_live[b] = res.n_live;
            if (cov) cvxr::covariance_problem(ln, pv.K, R_out + 9 * b, t_out + 3 * b, res.status, res.cost, res.n_live, o, cov + 36 * b);
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
