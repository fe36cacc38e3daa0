// grad_hip.hip -- device entry point of the pose VJP (include/cvxpnpl_amd_grad.h), built as libcvxpnpl_amd_grad.so.  The kernels are
// vjp_kernel.h, the mathematics vjp_core.h (shared with the host entry point, host_vjp.cpp, which is linked into the same library).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_grad.h"
#include "vjp_kernel.h"
#include "solver_entry.h"

using cvxse::fail; // (the error text, the correspondence block and the limit of one launch: solver_entry.h)
using cvxse::hip_error;
using cvxse::launched;

extern "C" const char *cvxpnpl_grad_last_error(void) { return cvxse::err_buf(); }

// (the order of the checks is that of the solver library's entry points, cvxpnpl_hip.hip: the arguments, the empty batch, the limits of one
// launch, the launches)
extern "C" int cvxpnpl_pose_vjp_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l, const double *d_line_2d,
                           const double *d_line_3d, const double *d_K, int32_t K_per_problem, const double *d_R, const double *d_t,
                           const int32_t *d_status, uint32_t admit_mask, const double *d_gR, const double *d_gt, double *d_g_pts_2d,
                           double *d_g_pts_3d, double *d_g_line_2d, double *d_g_line_3d, int32_t *d_vjp_status, double *d_vjp_info, void *stream)
{
    if (cvxse::bad_corr_block(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K) || (n_p == 0 && n_l == 0) ||
        (batch > 0 && (!d_R || !d_t || !d_vjp_status)))
        return fail(-1, "cvxpnpl_pose_vjp_batch: bad arguments (batch=%lld n_p=%d n_l=%d)", (long long)batch, n_p, n_l);
    if (batch == 0) return 0;
    cvxv::VjpArgs a;
    a.batch = batch; a.n_p = n_p; a.n_l = n_l; a.K_per_problem = K_per_problem; a.admit = admit_mask;
    a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.l2 = d_line_2d; a.l3 = d_line_3d; a.K = d_K; a.R = d_R; a.t = d_t; a.gR = d_gR; a.gt = d_gt;
    a.status = d_status; a.g2 = d_g_pts_2d; a.g3 = d_g_pts_3d; a.gl2 = d_g_line_2d; a.gl3 = d_g_line_3d; a.info = d_vjp_info; a.vstatus = d_vjp_status;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ncorr = (int64_t)n_p + n_l, nrec = (int64_t)n_p + 2 * (int64_t)n_l;
    if (nrec < cvxv::VJP_LARGE_N || batch > 65535) { // (more problems than one grid dimension holds: the group kernel loops over any N)
        const int64_t grid = (batch + cvxv::VJP_TPB / 16 - 1) / (cvxv::VJP_TPB / 16);
        if (cvxse::over_grid(grid, "cvxpnpl_pose_vjp_batch: batch too large for one launch")) return -1;
        if (d_vjp_info) hipLaunchKernelGGL(cvxv::vjp_group_kernel<true>, dim3((unsigned)grid), dim3(cvxv::VJP_TPB), 0, s, a);
        else hipLaunchKernelGGL(cvxv::vjp_group_kernel<false>, dim3((unsigned)grid), dim3(cvxv::VJP_TPB), 0, s, a);
        return launched("vjp_group_kernel launch");
    }
    // many correspondences per problem: partial sums in stream-ordered scratch, freed on the same stream
    if (cvxse::over_grid((batch * ncorr + cvxv::VJP_TPB - 1) / cvxv::VJP_TPB, "cvxpnpl_pose_vjp_batch: too many correspondences for one launch")) return -1;
    const int nblk = cvxv::vjp_blocks(ncorr, batch);
    const size_t part_bytes = (size_t)batch * nblk * cvxv::ACC_N * sizeof(double), bytes = part_bytes + (size_t)batch * cvxv::VJP_STRIDE * sizeof(double);
    void *scratch = nullptr;
    const hipError_t e = hipMallocAsync(&scratch, bytes, s);
    if (e != hipSuccess) return hip_error("cvxpnpl_pose_vjp_batch scratch", e);
    double *partial = (double *)scratch, *vs = (double *)((char *)scratch + part_bytes);
    hipLaunchKernelGGL(cvxv::vjp_reduce_kernel, dim3((unsigned)nblk, (unsigned)batch), dim3(cvxv::VJP_TPB), 0, s, a, nblk, partial);
    hipLaunchKernelGGL(cvxv::vjp_solve_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, a, nblk, partial, vs);
    hipLaunchKernelGGL(cvxv::vjp_scatter_kernel, dim3((unsigned)((batch * ncorr + cvxv::VJP_TPB - 1) / cvxv::VJP_TPB)), dim3(cvxv::VJP_TPB), 0, s, a, vs);
    const int rc = launched("vjp kernel launch");
    const hipError_t ef = hipFreeAsync(scratch, s); // (also after a failed launch)
    if (rc) return rc;
    return ef == hipSuccess ? 0 : hip_error("cvxpnpl_pose_vjp_batch scratch", ef);
}
