// host_refine_vjp.cpp -- host entry point of the refinement's backward pass (cvxpnpl_refine_vjp_batch_host): a threaded loop over the same
// core (refine_vjp_core.h) as the device kernels (refine_vjp_kernel.h), so that the CPU test suite reaches the same mathematics.  The
// argument contract and the error text are refine_entry.h's; check_common holds what is this library's own, for the device entry points
// (refine_grad_hip.hip, linked into the same library) too.
#include "../../include/cvxpnpl_amd_refine_grad.h"
#include "refine_entry.h"
#include "refine_vjp_core.h"

namespace cvxrg {

// K and the poses, the status output, the status column: what the three entry points check once the sizes are known to be positive
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t,
                                                       const int32_t *status, int64_t status_stride, const void *vjp_status)
{
    if (const char *m = cvxre::check_pose(K_per, K, R, t)) return cvxre::bad_args(who, m);
    if (!vjp_status) return cvxre::bad_args(who, "vjp_status is null");
    if (const char *m = cvxre::check_status(status, status_stride)) return cvxre::bad_args(who, m);
    return 0;
}

} // namespace cvxrg

extern "C" const char *cvxpnpl_refine_grad_last_error(void) { return cvxre::err_buf(); }

extern "C" const char *cvxpnpl_refine_grad_version(void) { return "cvxpnpl_amd_refine_grad 1"; }

extern "C" int cvxpnpl_refine_vjp_batch_host(int64_t batch, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                             const double *line_3d, const double *K, int32_t K_per_problem, const double *R, const double *t,
                                             const int32_t *refine_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts,
                                             const uint8_t *mask_lines, const double *grad_R, const double *grad_t, double *g_pts_2d, double *g_pts_3d,
                                             double *g_line_2d, double *g_line_3d, int32_t *vjp_status, double *info, int32_t n_threads)
{
    const char *who = "cvxpnpl_refine_vjp_batch_host";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, pts_2d, pts_3d, n_l, line_2d, line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxrg::check_common(who, K_per_problem, K, R, t, refine_status, status_stride, vjp_status)) return rc;
    cvxh::for_chunks(batch, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            cvxr::HostLanes ln;
            bool admit;
            const double *Kb = cvxre::host_problem(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, refine_status, status_stride,
                                                   admit_mask, mask_pts, mask_lines, ln.pb, admit);
            cvxrg::Grads g;
            cvxre::host_grads(g, b, n_p, n_l, g_pts_2d, g_pts_3d, g_line_2d, g_line_3d);
            vjp_status[b] = cvxrg::vjp_problem(ln, 0, 1, Kb, R + 9 * b, t + 3 * b, grad_R ? grad_R + 9 * b : nullptr, grad_t ? grad_t + 3 * b : nullptr,
                                               admit, true, g, info ? info + 2 * b : nullptr);
        }
    });
    return 0;
}
