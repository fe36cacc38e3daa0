// host_refine_robust_vjp.cpp -- host entry point of the robust refinement's backward pass (cvxpnpl_refine_robust_vjp_batch_host): a
// threaded loop over the same core (refine_robust_vjp_core.h) as the device kernels (refine_robust_vjp_kernel.h), so that the CPU test
// suite reaches the same mathematics.  Also the argument checks and the error text that the device entry points
// (refine_robust_grad_hip.hip, linked into the same library) share with it.
#include <algorithm>
#include <cmath>
#include <stdio.h>
#include <thread>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_robust_grad.h"
#include "refine_robust_vjp_core.h"

namespace cvxrbg {

// (hidden: the library exports what its header declares and nothing else; refine_robust_grad_hip.hip declares the same three)
__attribute__((visibility("hidden"))) char *err_buf();
__attribute__((visibility("hidden"))) int bad_args(const char *who, const char *what);
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t,
                                                       const int32_t *status, int64_t status_stride, int32_t loss, double scale_px,
                                                       const void *vjp_status);

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

// what the three entry points share once the sizes are known to be positive
int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status, int64_t status_stride,
                 int32_t loss, double scale_px, const void *vjp_status)
{
    if (K_per != 0 && K_per != 1) return bad_args(who, "K_per_problem / K_per_scene is 0 or 1");
    if (!K || !R || !t) return bad_args(who, "K, R or t is null");
    if (!vjp_status) return bad_args(who, "vjp_status is null");
    if (status && status_stride < 0) return bad_args(who, "negative status_stride");
    if (loss < cvxrb::LOSS_L2 || loss > cvxrb::LOSS_CAUCHY) return bad_args(who, "loss is 0 (l2), 1 (huber) or 2 (cauchy)");
    if (loss != cvxrb::LOSS_L2 && (!(scale_px > 0.0) || !std::isfinite(scale_px))) return bad_args(who, "scale_px is not a finite positive number");
    return 0;
}

} // namespace cvxrbg

extern "C" const char *cvxpnpl_refine_robust_grad_last_error(void) { return cvxrbg::err_buf(); }

extern "C" const char *cvxpnpl_refine_robust_grad_version(void) { return "cvxpnpl_amd_refine_robust_grad 1"; }

extern "C" int cvxpnpl_refine_robust_vjp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l,
                                                    const double *line_2d, const double *line_3d, const double *K, int32_t K_per_problem,
                                                    const double *R, const double *t, const int32_t *refine_status, int64_t status_stride,
                                                    uint32_t admit_mask, int32_t loss, double scale_px, const uint8_t *mask_pts,
                                                    const uint8_t *mask_lines, const double *w_pts, const double *w_lines, const double *grad_R,
                                                    const double *grad_t, double *g_pts_2d, double *g_pts_3d, double *g_line_2d, double *g_line_3d,
                                                    double *g_w_pts, double *g_w_lines, int32_t *vjp_status, double *info, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_robust_vjp_batch_host";
    if (batch < 0 || n_p < 0 || n_l < 0 || (int64_t)n_p + n_l > 0x7fffffffLL) return cvxrbg::bad_args(who, "negative size");
    if (batch == 0) return 0;
    if ((n_p > 0 && (!pts_2d || !pts_3d)) || (n_l > 0 && (!line_2d || !line_3d))) return cvxrbg::bad_args(who, "a correspondence pointer is null");
    if (int rc = cvxrbg::check_common(who, K_per_problem, K, R, t, refine_status, status_stride, loss, scale_px, vjp_status)) return rc;
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
            wp.ow_p = g_w_pts && n_p > 0 ? g_w_pts + b * n_p : nullptr; // (the weights' gradients: refine_robust_vjp_core.h)
            wp.ow_l = g_w_lines && n_l > 0 ? g_w_lines + b * n_l : nullptr;
            const bool admit = !refine_status || cvxr::admitted(refine_status[b * status_stride], admit_mask);
            cvxrg::Grads g;
            g.p2 = g_pts_2d && n_p > 0 ? g_pts_2d + b * n_p * 2 : nullptr;
            g.p3 = g_pts_3d && n_p > 0 ? g_pts_3d + b * n_p * 3 : nullptr;
            g.l2 = g_line_2d && n_l > 0 ? g_line_2d + b * n_l * 4 : nullptr;
            g.l3 = g_line_3d && n_l > 0 ? g_line_3d + b * n_l * 6 : nullptr;
            vjp_status[b] = cvxrbg::robust_vjp_problem(ln, wp, pv.K, R + 9 * b, t + 3 * b, grad_R ? grad_R + 9 * b : nullptr,
                                                       grad_t ? grad_t + 3 * b : nullptr, admit, true, l, g, info ? info + 2 * b : nullptr);
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
