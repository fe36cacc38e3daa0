// refine_robust_auto_hip.hip -- device entry points of the twelfth library (include/cvxpnpl_amd_refine_robust_auto.h), built as
// libcvxpnpl_amd_refine_robust_auto.so.  The kernels are refine_robust_auto_kernel.h, the mathematics refine_robust_auto_core.h (shared
// with the host entry points, host_refine_robust_auto.cpp, which is linked into the same library).  The argument contract is
// refine_entry.h's, the library's own checks host_refine_robust_auto.cpp's.  Every entry point checks its arguments before it launches
// anything.
#include <hip/hip_runtime.h>

#include "../../include/cvxpnpl_amd_refine_robust_auto.h"
#include "refine_entry.h"
#include "refine_robust_auto_kernel.h"

namespace cvxra {

// (defined in host_refine_robust_auto.cpp)
__attribute__((visibility("hidden"))) int check_scale(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                      int64_t status_stride, const void *sigma, const void *med_sq, const void *n_live, const void *status_out,
                                                      bool sq_given);
__attribute__((visibility("hidden"))) int check_loop(const char *who, int32_t K_per, const double *K, const double *R, const double *t, const int32_t *status,
                                                     int64_t status_stride, const cvxpnpl_refine_robust_opts_t *opts, const void *R_out, const void *t_out,
                                                     const void *cost, const void *iters, const void *status_out, const void *n_live, const void *n_inlier,
                                                     cvxr::Opts &o, int &loss, double &scale_px);
__attribute__((visibility("hidden"))) int check_cov(const char *who, int32_t K_per, const double *K, const double *R, const double *t, int32_t loss, double scale_px,
                                                    const double *scale_each, const void *cov, const void *cov_status);

// what a call does not use of the argument blocks
template <class A>
static void clear(A &pa)
{
    pa.a.opts = cvxr::Opts{0, 0.0, 0.0, 0.0};
    pa.a.loss_kind = 0; pa.a.scale_px = 1.0;
    pa.a.wp = pa.a.wl = nullptr;
    pa.a.out = cvxrb::Outputs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    pa.scale = nullptr; pa.sigma = pa.med_sq = pa.cov = nullptr; pa.cov_status = nullptr;
}

} // namespace cvxra

extern "C" int cvxpnpl_robust_scale_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                          const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                          const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                          const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, double *d_sigma, double *d_med_sq,
                                          int32_t *d_n_live, int32_t *d_status_out, double *d_sq, void *stream)
{
    const char *who = "cvxpnpl_robust_scale_batch";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_scale(who, K_per_problem, d_K, d_R, d_t, d_status, status_stride, d_sigma, d_med_sq, d_n_live, d_status_out, d_sq || n_p + n_l == 0))
        return rc;
    int64_t grid;
    if (const char *m = cvxre::check_batch_grid(batch, cvxra::TPB / 16, grid)) return cvxre::bad_args(who, m);
    cvxra::AutoBatchArgs pa;
    cvxra::clear(pa);
    cvxre::fill_batch(pa.a, batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem, d_R, d_t, d_status, status_stride, admit_mask,
                      d_mask_pts, d_mask_lines);
    pa.a.wp = n_p > 0 ? d_w_pts : nullptr; pa.a.wl = n_l > 0 ? d_w_lines : nullptr;
    pa.a.out.status = d_status_out; pa.a.out.n_live = d_n_live; pa.a.out.rw_p = d_sq;
    pa.sigma = d_sigma; pa.med_sq = d_med_sq;
    const int ncorr = n_p + n_l;
    const dim3 g((unsigned)grid), blk(cvxra::TPB);
    hipStream_t s = (hipStream_t)stream;
    // records per lane held in registers with their s_k through every round: 1, 2 or 4; beyond 64 correspondences every round reads sq again
    if (ncorr <= 16) hipLaunchKernelGGL(cvxra::robust_scale_group_kernel<1>, g, blk, 0, s, pa);
    else if (ncorr <= 32) hipLaunchKernelGGL(cvxra::robust_scale_group_kernel<2>, g, blk, 0, s, pa);
    else if (ncorr <= 64) hipLaunchKernelGGL(cvxra::robust_scale_group_kernel<4>, g, blk, 0, s, pa);
    else hipLaunchKernelGGL(cvxra::robust_scale_group_kernel<0>, g, blk, 0, s, pa);
    return cvxre::launched("robust_scale_group_kernel launch");
}

extern "C" int cvxpnpl_robust_scale_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                           const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                                           int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status, int64_t status_stride,
                                           uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_w_pts,
                                           const double *d_w_lines, double *d_sigma, double *d_med_sq, int32_t *d_n_live, int32_t *d_status_out,
                                           double *d_sq_pts, double *d_sq_lines, void *stream)
{
    const char *who = "cvxpnpl_robust_scale_scenes";
    if (const char *m = cvxre::check_sizes(n_scenes, n_pts, n_lines)) return cvxre::bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = cvxre::check_scenes(d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d))
        return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_scale(who, K_per_scene, d_K, d_R, d_t, d_status, status_stride, d_sigma, d_med_sq, d_n_live, d_status_out,
                                    (d_sq_pts || n_pts == 0) && (d_sq_lines || n_lines == 0)))
        return rc;
    if (const char *m = cvxre::check_scenes_grid(n_scenes)) return cvxre::bad_args(who, m);
    cvxra::AutoSceneArgs pa;
    cvxra::clear(pa);
    cvxre::fill_scenes(pa.a, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, d_K, K_per_scene, d_R, d_t,
                       d_status, status_stride, admit_mask, d_mask_pts, d_mask_lines);
    pa.a.wp = n_pts > 0 ? d_w_pts : nullptr; pa.a.wl = n_lines > 0 ? d_w_lines : nullptr;
    pa.a.out.status = d_status_out; pa.a.out.n_live = d_n_live;
    pa.a.out.rw_p = n_pts > 0 ? d_sq_pts : nullptr; pa.a.out.rw_l = n_lines > 0 ? d_sq_lines : nullptr;
    pa.sigma = d_sigma; pa.med_sq = d_med_sq;
    hipLaunchKernelGGL(cvxra::robust_scale_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxra::TPB), 0, (hipStream_t)stream, pa);
    return cvxre::launched("robust_scale_scenes_kernel launch");
}

extern "C" int cvxpnpl_refine_robust_pp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                              const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                              const int32_t *d_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                              const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, const double *d_scale_px,
                                              const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                              int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w, int32_t *d_n_inlier, void *stream)
{
    const char *who = "cvxpnpl_refine_robust_pp_batch";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d)) return cvxre::bad_args(who, m);
    cvxra::AutoBatchArgs pa;
    cvxra::clear(pa);
    cvxrb::BatchArgs &a = pa.a;
    if (int rc = cvxra::check_loop(who, K_per_problem, d_K, d_R, d_t, d_status, status_stride, opts, d_R_out, d_t_out, d_cost, d_iters, d_status_out, d_n_live,
                                   d_n_inlier, a.opts, a.loss_kind, a.scale_px))
        return rc;
    int64_t grid;
    if (const char *m = cvxre::check_batch_grid(batch, cvxra::TPB / 16, grid)) return cvxre::bad_args(who, m);
    cvxre::fill_batch(a, batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem, d_R, d_t, d_status, status_stride, admit_mask,
                      d_mask_pts, d_mask_lines);
    a.wp = n_p > 0 ? d_w_pts : nullptr; a.wl = n_l > 0 ? d_w_lines : nullptr;
    a.out.R = d_R_out; a.out.t = d_t_out; a.out.cost = d_cost; a.out.iters = d_iters; a.out.status = d_status_out; a.out.n_live = d_n_live;
    a.out.n_inlier = d_n_inlier; a.out.rw_p = d_robust_w; a.out.rw_l = nullptr;
    pa.scale = a.loss_kind == CVXPNPL_LOSS_L2 ? nullptr : d_scale_px; // (l2 does not read it)
    const int ncorr = n_p + n_l;
    const dim3 g((unsigned)grid), blk(cvxra::TPB);
    hipStream_t s = (hipStream_t)stream;
    if (ncorr <= 16) hipLaunchKernelGGL(cvxra::refine_robust_pp_group_kernel<1>, g, blk, 0, s, pa);
    else if (ncorr <= 32) hipLaunchKernelGGL(cvxra::refine_robust_pp_group_kernel<2>, g, blk, 0, s, pa);
    else if (ncorr <= 64) hipLaunchKernelGGL(cvxra::refine_robust_pp_group_kernel<4>, g, blk, 0, s, pa);
    else hipLaunchKernelGGL(cvxra::refine_robust_pp_group_kernel<0>, g, blk, 0, s, pa);
    hipLaunchKernelGGL(cvxra::robust_w_pp_group_kernel, g, blk, 0, s, pa); // (reads what the launch before it wrote)
    return cvxre::launched("refine_robust_pp_group_kernel launch");
}

extern "C" int cvxpnpl_refine_robust_pp_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                               const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                               const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status,
                                               int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                                               const double *d_w_pts, const double *d_w_lines, const double *d_scale_px,
                                               const cvxpnpl_refine_robust_opts_t *opts, double *d_R_out, double *d_t_out, double *d_cost, int32_t *d_iters,
                                               int32_t *d_status_out, int32_t *d_n_live, double *d_robust_w_pts, double *d_robust_w_lines,
                                               int32_t *d_n_inlier, void *stream)
{
    const char *who = "cvxpnpl_refine_robust_pp_scenes";
    if (const char *m = cvxre::check_sizes(n_scenes, n_pts, n_lines)) return cvxre::bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = cvxre::check_scenes(d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d))
        return cvxre::bad_args(who, m);
    cvxra::AutoSceneArgs pa;
    cvxra::clear(pa);
    cvxrb::SceneArgs &a = pa.a;
    if (int rc = cvxra::check_loop(who, K_per_scene, d_K, d_R, d_t, d_status, status_stride, opts, d_R_out, d_t_out, d_cost, d_iters, d_status_out, d_n_live,
                                   d_n_inlier, a.opts, a.loss_kind, a.scale_px))
        return rc;
    if (const char *m = cvxre::check_scenes_grid(n_scenes)) return cvxre::bad_args(who, m);
    cvxre::fill_scenes(a, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, d_K, K_per_scene, d_R, d_t,
                       d_status, status_stride, admit_mask, d_mask_pts, d_mask_lines);
    a.wp = n_pts > 0 ? d_w_pts : nullptr; a.wl = n_lines > 0 ? d_w_lines : nullptr;
    a.out.R = d_R_out; a.out.t = d_t_out; a.out.cost = d_cost; a.out.iters = d_iters; a.out.status = d_status_out; a.out.n_live = d_n_live;
    a.out.n_inlier = d_n_inlier; a.out.rw_p = n_pts > 0 ? d_robust_w_pts : nullptr; a.out.rw_l = n_lines > 0 ? d_robust_w_lines : nullptr;
    pa.scale = a.loss_kind == CVXPNPL_LOSS_L2 ? nullptr : d_scale_px;
    const dim3 g((unsigned)n_scenes), blk(cvxra::TPB);
    hipLaunchKernelGGL(cvxra::refine_robust_pp_scenes_kernel, g, blk, 0, (hipStream_t)stream, pa);
    hipLaunchKernelGGL(cvxra::robust_w_pp_scenes_kernel, g, blk, 0, (hipStream_t)stream, pa); // (reads what the launch before it wrote)
    return cvxre::launched("refine_robust_pp_scenes_kernel launch");
}

extern "C" int cvxpnpl_robust_cov_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                        const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                        const int32_t *d_status, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_w_pts,
                                        const double *d_w_lines, int32_t loss, double scale_px, const double *d_scale_px, double *d_cov, int32_t *d_cov_status,
                                        void *stream)
{
    const char *who = "cvxpnpl_robust_cov_batch";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_cov(who, K_per_problem, d_K, d_R, d_t, loss, scale_px, d_scale_px, d_cov, d_cov_status)) return rc;
    int64_t grid;
    if (const char *m = cvxre::check_batch_grid(batch, cvxra::TPB / 16, grid)) return cvxre::bad_args(who, m);
    cvxra::AutoBatchArgs pa;
    cvxra::clear(pa);
    cvxre::fill_batch(pa.a, batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem, d_R, d_t, d_status, 1, 0u, d_mask_pts, d_mask_lines);
    pa.a.wp = n_p > 0 ? d_w_pts : nullptr; pa.a.wl = n_l > 0 ? d_w_lines : nullptr;
    pa.a.loss_kind = loss; pa.a.scale_px = loss == CVXPNPL_LOSS_L2 ? 1.0 : scale_px;
    pa.scale = loss == CVXPNPL_LOSS_L2 ? nullptr : d_scale_px;
    pa.cov = d_cov; pa.cov_status = d_cov_status;
    hipLaunchKernelGGL(cvxra::robust_cov_group_kernel, dim3((unsigned)grid), dim3(cvxra::TPB), 0, (hipStream_t)stream, pa);
    return cvxre::launched("robust_cov_group_kernel launch");
}

extern "C" int cvxpnpl_robust_cov_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                         const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d, const double *d_K,
                                         int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_status, const uint8_t *d_mask_pts,
                                         const uint8_t *d_mask_lines, const double *d_w_pts, const double *d_w_lines, int32_t loss, double scale_px,
                                         const double *d_scale_px, double *d_cov, int32_t *d_cov_status, void *stream)
{
    const char *who = "cvxpnpl_robust_cov_scenes";
    if (const char *m = cvxre::check_sizes(n_scenes, n_pts, n_lines)) return cvxre::bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = cvxre::check_scenes(d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d))
        return cvxre::bad_args(who, m);
    if (int rc = cvxra::check_cov(who, K_per_scene, d_K, d_R, d_t, loss, scale_px, d_scale_px, d_cov, d_cov_status)) return rc;
    if (const char *m = cvxre::check_scenes_grid(n_scenes)) return cvxre::bad_args(who, m);
    cvxra::AutoSceneArgs pa;
    cvxra::clear(pa);
    cvxre::fill_scenes(pa.a, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, d_K, K_per_scene, d_R, d_t,
                       d_status, 1, 0u, d_mask_pts, d_mask_lines);
    pa.a.wp = n_pts > 0 ? d_w_pts : nullptr; pa.a.wl = n_lines > 0 ? d_w_lines : nullptr;
    pa.a.loss_kind = loss; pa.a.scale_px = loss == CVXPNPL_LOSS_L2 ? 1.0 : scale_px;
    pa.scale = loss == CVXPNPL_LOSS_L2 ? nullptr : d_scale_px;
    pa.cov = d_cov; pa.cov_status = d_cov_status;
    hipLaunchKernelGGL(cvxra::robust_cov_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxra::TPB), 0, (hipStream_t)stream, pa);
    return cvxre::launched("robust_cov_scenes_kernel launch");
}
