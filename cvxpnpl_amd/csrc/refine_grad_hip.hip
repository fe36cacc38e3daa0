// refine_grad_hip.hip -- device entry points of the refinement's backward pass (include/cvxpnpl_amd_refine_grad.h), built as
// libcvxpnpl_amd_refine_grad.so.  The kernels are refine_vjp_kernel.h, the mathematics refine_vjp_core.h (shared with the host entry
// point, host_refine_vjp.cpp, which is linked into the same library).  The argument contract is refine_entry.h's, the library's own checks
// host_refine_vjp.cpp's check_common.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>

#include "../../include/cvxpnpl_amd_refine_grad.h"
#include "refine_entry.h"
#include "refine_vjp_kernel.h"

namespace cvxrg {

// (defined in host_refine_vjp.cpp)
__attribute__((visibility("hidden"))) int check_common(const char *who, int32_t K_per, const double *K, const double *R, const double *t,
                                                       const int32_t *status, int64_t status_stride, const void *vjp_status);

} // namespace cvxrg

extern "C" int cvxpnpl_refine_vjp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                                        const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                                        const int32_t *d_refine_status, int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts,
                                        const uint8_t *d_mask_lines, const double *d_grad_R, const double *d_grad_t, double *d_g_pts_2d,
                                        double *d_g_pts_3d, double *d_g_line_2d, double *d_g_line_3d, int32_t *d_vjp_status, double *d_info, void *stream)
{
    const char *who = "cvxpnpl_refine_vjp_batch";
    if (const char *m = cvxre::check_sizes(batch, n_p, n_l, INT32_MAX)) return cvxre::bad_args(who, m);
    if (batch == 0) return 0;
    if (const char *m = cvxre::check_pairs(n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d)) return cvxre::bad_args(who, m);
    if (int rc = cvxrg::check_common(who, K_per_problem, d_K, d_R, d_t, d_refine_status, status_stride, d_vjp_status)) return rc;
    int64_t grid;
    if (const char *m = cvxre::check_batch_grid(batch, cvxr::TPB / 16, grid)) return cvxre::bad_args(who, m);
    cvxrg::VjpBatchArgs a;
    cvxre::fill_batch(a, batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem, d_R, d_t, d_refine_status, status_stride,
                      admit_mask, d_mask_pts, d_mask_lines);
    a.gR = d_grad_R; a.gt = d_grad_t;
    a.g_p2 = n_p > 0 ? d_g_pts_2d : nullptr; a.g_p3 = n_p > 0 ? d_g_pts_3d : nullptr;
    a.g_l2 = n_l > 0 ? d_g_line_2d : nullptr; a.g_l3 = n_l > 0 ? d_g_line_3d : nullptr;
    a.info = d_info; a.vstatus = d_vjp_status;
    const int64_t ncorr = (int64_t)n_p + n_l;
    const dim3 g((unsigned)grid), blk(cvxr::TPB);
    hipStream_t s = (hipStream_t)stream;
    // records per lane held in registers between the two passes: 1, 2 or 4; beyond 64 correspondences the second pass reads them again
    if (ncorr <= 16) hipLaunchKernelGGL(cvxrg::refine_vjp_group_kernel<1>, g, blk, 0, s, a);
    else if (ncorr <= 32) hipLaunchKernelGGL(cvxrg::refine_vjp_group_kernel<2>, g, blk, 0, s, a);
    else if (ncorr <= 64) hipLaunchKernelGGL(cvxrg::refine_vjp_group_kernel<4>, g, blk, 0, s, a);
    else hipLaunchKernelGGL(cvxrg::refine_vjp_group_kernel<0>, g, blk, 0, s, a);
    return cvxre::launched("refine_vjp_group_kernel launch");
}

extern "C" int cvxpnpl_refine_vjp_scenes(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                         const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                         const double *d_K, int32_t K_per_scene, const double *d_R, const double *d_t, const int32_t *d_refine_status,
                                         int64_t status_stride, uint32_t admit_mask, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines,
                                         const double *d_grad_R, const double *d_grad_t, double *d_g_pts_2d, double *d_g_pts_3d, double *d_g_line_2d,
                                         double *d_g_line_3d, int32_t *d_vjp_status, double *d_info, void *stream)
{
    const char *who = "cvxpnpl_refine_vjp_scenes";
    if (const char *m = cvxre::check_sizes(n_scenes, n_pts, n_lines)) return cvxre::bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = cvxre::check_scenes(d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d))
        return cvxre::bad_args(who, m);
    if (int rc = cvxrg::check_common(who, K_per_scene, d_K, d_R, d_t, d_refine_status, status_stride, d_vjp_status)) return rc;
    if (const char *m = cvxre::check_scenes_grid(n_scenes)) return cvxre::bad_args(who, m);
    cvxrg::VjpSceneArgs a;
    cvxre::fill_scenes(a, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, d_K, K_per_scene, d_R, d_t,
                       d_refine_status, status_stride, admit_mask, d_mask_pts, d_mask_lines);
    a.gR = d_grad_R; a.gt = d_grad_t;
    a.g_p2 = n_pts > 0 ? d_g_pts_2d : nullptr; a.g_p3 = n_pts > 0 ? d_g_pts_3d : nullptr;
    a.g_l2 = n_lines > 0 ? d_g_line_2d : nullptr; a.g_l3 = n_lines > 0 ? d_g_line_3d : nullptr;
    a.info = d_info; a.vstatus = d_vjp_status;
    hipLaunchKernelGGL(cvxrg::refine_vjp_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxr::TPB), 0, (hipStream_t)stream, a);
    return cvxre::launched("refine_vjp_scenes_kernel launch");
}
