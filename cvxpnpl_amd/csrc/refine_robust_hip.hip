// refine_robust_hip.hip -- device entry points of the robust reprojection refinement (include/cvxpnpl_amd_refine_robust.h), built as
// libcvxpnpl_amd_refine_robust.so.  The kernels are refine_robust_kernel.h, the mathematics refine_robust_core.h (shared with the host
// entry point, host_refine_robust.cpp, which is linked into the same library).  The argument contract is refine_entry.h's, the library's
// own checks host_refine_robust.cpp's check_common.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>

#include "../../include/cvxpnpl_amd_refine_robust.h"
#include "refine_entry.h"
#include "refine_robust_kernel.h"

namespace cvxrb {

// (defined in host_refine_robust.cpp)
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                       int64_t status_stride, const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out,
                                                       const void *cost, const void *iters, const void *status_out, const void *n_live,
                                                       const void *n_inlier, Opts &o, int &loss, double &scale_px);

} // namespace cvxrb

extern "C" int cvxpnpl_refine_robust_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                           const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                           const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                           const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines,
                                           const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                           int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w, int32_t *d_n_inlier, void *stream)
{
    const char *who = "cvxpnpl_refine_robust_batch";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d)) return cvxre::bad_args(who, m);
    cvxrb::BatchArgs a;
    if (int rc = cvxrb::check_common(who, K_per_problem, d_K, d_R, d_t, d_status, status_stride, opts, d_R_out, d_t_out, d_cost, d_iters, d_status_out,
                                     d_n_live, d_n_inlier, a.opts, a.loss_kind, a.scale_px))
        return rc;
    int64_t grid;
    if (const char *m = cvxre::check_batch_grid(batch, cvxrb::TPB / 16, grid)) return cvxre::bad_args(who, m);
    cvxre::fill_batch(a, batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem, d_R, d_t, d_status, status_stride, admit_mask,
                      d_mask_pts, d_mask_lines);
    a.wp = n_p > 0 ? d_w_pts : nullptr; a.wl = n_l > 0 ? d_w_lines : nullptr;
    a.out.R = d_R_out; a.out.t = d_t_out; a.out.cost = d_cost; a.out.iters = d_iters; a.out.status = d_status_out; a.out.n_live = d_n_live;
    a.out.n_inlier = d_n_inlier; a.out.rw_p = d_robust_w; a.out.rw_l = nullptr;
    const int ncorr = n_p + n_l;
    const dim3 g((unsigned)grid), blk(cvxrb::TPB);
    hipStream_t s = (hipStream_t)stream;
    // records per lane held in registers with their weights: 1, 2 or 4; beyond 64 correspondences every pass reads them again
    if (ncorr <= 16) hipLaunchKernelGGL(cvxrb::refine_robust_group_kernel<1>, g, blk, 0, s, a);
    else if (ncorr <= 32) hipLaunchKernelGGL(cvxrb::refine_robust_group_kernel<2>, g, blk, 0, s, a);
    else if (ncorr <= 64) hipLaunchKernelGGL(cvxrb::refine_robust_group_kernel<4>, g, blk, 0, s, a);
    else hipLaunchKernelGGL(cvxrb::refine_robust_group_kernel<0>, g, blk, 0, s, a);
    hipLaunchKernelGGL(cvxrb::robust_w_group_kernel, g, blk, 0, s, a); // (reads what the launch before it wrote)
    return cvxre::launched("refine_robust_group_kernel launch");
}

extern "C" int cvxpnpl_refine_robust_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                            const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                            const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status,
                                            int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                                            const double *d_w_pts, const double *d_w_lines, const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out,
                                            double *d_t_out, double *d_cost, int32_t *d_iters, int32_t *d_status_out, int32_t *d_n_live,
                                            double *d_robust_w_pts, double *d_robust_w_lines, int32_t *d_n_inlier, void *stream)
{
    const char *who = "cvxpnpl_refine_robust_scenes";
    if (const char *m = cvxre::check_sizes(n_scenes, n_pts, n_lines)) return cvxre::bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = cvxre::check_scenes(d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d))
        return cvxre::bad_args(who, m);
    cvxrb::SceneArgs a;
    if (int rc = cvxrb::check_common(who, K_per_scene, d_K, d_R, d_t, d_status, status_stride, opts, d_R_out, d_t_out, d_cost, d_iters, d_status_out, d_n_live,
                                     d_n_inlier, a.opts, a.loss_kind, a.scale_px))
        return rc;
    if (const char *m = cvxre::check_scenes_grid(n_scenes)) return cvxre::bad_args(who, m);
    cvxre::fill_scenes(a, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, d_K, K_per_scene, d_R, d_t,
                       d_status, status_stride, admit_mask, d_mask_pts, d_mask_lines);
    a.wp = n_pts > 0 ? d_w_pts : nullptr; a.wl = n_lines > 0 ? d_w_lines : nullptr;
    a.out.R = d_R_out; a.out.t = d_t_out; a.out.cost = d_cost; a.out.iters = d_iters; a.out.status = d_status_out; a.out.n_live = d_n_live;
    a.out.n_inlier = d_n_inlier; a.out.rw_p = n_pts > 0 ? d_robust_w_pts : nullptr; a.out.rw_l = n_lines > 0 ? d_robust_w_lines : nullptr;
    const dim3 g((unsigned)n_scenes), blk(cvxrb::TPB);
    hipLaunchKernelGGL(cvxrb::refine_robust_scenes_kernel, g, blk, 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(cvxrb::robust_w_scenes_kernel, g, blk, 0, (hipStream_t)stream, a); // (reads what the launch before it wrote)
    return cvxre::launched("refine_robust_scenes_kernel launch");
}
