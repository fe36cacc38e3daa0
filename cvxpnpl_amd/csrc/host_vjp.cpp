// host_vjp.cpp -- host entry point of the pose VJP (cvxpnpl_pose_vjp_host): a threaded loop over the same core (vjp_core.h) as the
// device kernels (vjp_kernel.h), so that the CPU test suite can check the mathematics against finite differences.
#include <algorithm>

#include "../../include/cvxpnpl_amd_grad.h"
#include "host_pool.h"
#include "vjp_core.h"

namespace {

void zero_problem(int64_t b, int32_t n_p, int32_t n_l, double *g2, double *g3, double *gl2, double *gl3)
{
    if (g2) std::fill(g2 + b * n_p * 2, g2 + (b + 1) * n_p * 2, 0.0);
    if (g3) std::fill(g3 + b * n_p * 3, g3 + (b + 1) * n_p * 3, 0.0);
    if (gl2) std::fill(gl2 + b * n_l * 4, gl2 + (b + 1) * n_l * 4, 0.0);
    if (gl3) std::fill(gl3 + b * n_l * 6, gl3 + (b + 1) * n_l * 6, 0.0);
}

} // namespace

extern "C" int cvxpnpl_pose_vjp_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                     const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                     const int32_t *status, uint32_t admit_mask, const double *gR, const double *gt, double *g_pts_2d,
                                     double *g_pts_3d, double *g_line_2d, double *g_line_3d, int32_t *vjp_status, double *vjp_info, int32_t n_threads)
{
    if (batch < 0 || n_p < 0 || n_l < 0 || (n_p == 0 && n_l == 0) || !K || !R || !t || !vjp_status || (n_p > 0 && (!pts_2d || !pts_3d)) ||
        (n_l > 0 && (!line_2d || !line_3d)))
        return -1;
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            const cvx::ProblemView pv = cvx::make_view(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem);
            double info[2] = {NAN, NAN};
            if (vjp_info) { vjp_info[2 * b] = NAN; vjp_info[2 * b + 1] = NAN; }
            if (status && !cvxv::admitted(status[b], admit_mask)) {
                vjp_status[b] = cvxv::VJP_SKIPPED;
                zero_problem(b, n_p, n_l, g_pts_2d, g_pts_3d, g_line_2d, g_line_3d);
                continue;
            }
            cvxv::Frame fr;
            cvxv::frame_make(pv, R + 9 * b, t + 3 * b, fr);
            cvxv::Acc acc;
            cvxv::acc_zero(acc);
            for (int i = 0; i < n_p; ++i) cvxv::acc_point(acc, fr, pv.p2 + 2 * i, pv.p3 + 3 * i);
            for (int i = 0; i < n_l; ++i) cvxv::acc_line(acc, fr, pv.l2 + 4 * i, pv.l3 + 6 * i);
            double v[6];
            const int st = cvxv::solve_v(acc, fr, n_p + n_l, gR ? gR + 9 * b : nullptr, gt ? gt + 3 * b : nullptr, v, info, vjp_info != nullptr);
            if (vjp_info) { vjp_info[2 * b] = info[0]; vjp_info[2 * b + 1] = info[1]; }
            vjp_status[b] = st;
            if (st != cvxv::VJP_OK) {
                zero_problem(b, n_p, n_l, g_pts_2d, g_pts_3d, g_line_2d, g_line_3d);
                continue;
            }
            for (int i = 0; i < n_p; ++i)
                cvxv::vjp_point(fr, v, pv.p2 + 2 * i, pv.p3 + 3 * i, g_pts_2d ? g_pts_2d + (b * n_p + i) * 2 : nullptr,
                                g_pts_3d ? g_pts_3d + (b * n_p + i) * 3 : nullptr);
            for (int i = 0; i < n_l; ++i)
                cvxv::vjp_line(fr, v, pv.l2 + 4 * i, pv.l3 + 6 * i, g_line_2d ? g_line_2d + (b * n_l + i) * 4 : nullptr,
                               g_line_3d ? g_line_3d + (b * n_l + i) * 6 : nullptr);
        }
    });
    return 0;
}
