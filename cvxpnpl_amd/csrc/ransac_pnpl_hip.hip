// ransac_pnpl_hip.hip -- entry points of RANSAC over points and lines, many scenes (include/cvxpnpl_amd_ransac_pnpl.h), built as
// libcvxpnpl_amd_ransac_pnpl.so.  The kernels are ransac_pnpl_kernel.h, the shared checks and the slab launch ransac_entry.h.  Every entry
// point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_pnpl.h"
#include "ransac_entry.h"
#include "ransac_pnpl_kernel.h"

using namespace cvxne;

extern "C" const char *cvxpnpl_ransac_pnpl_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_pnpl_sample_assemble(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                                   int64_t n_lines, const uint64_t *d_seeds, const double *d_pts_2d, const double *d_pts_3d,
                                                   const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_scene, int32_t *d_idx,
                                                   double *d_Q45, double *d_B27, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_sample_assemble";
    cvxnl::SampleArgs a;
    if (const char *m = check_pnpl_scenes(false, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_seeds || !d_K || !d_Q45 || !d_B27) return bad_args(who, "d_seeds, d_K, d_Q45 or d_B27 is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.seed = d_seeds; a.idx = d_idx; a.Q45 = d_Q45; a.B27 = d_B27;
    launch_slabs(cvxnl::sample_assemble_kernel, n_hyp, cvxnl::BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("sample_assemble_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_score(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                         int64_t n_lines, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                         const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                         const double *d_line_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_score";
    cvxnl::ScoreArgs a;
    if (const char *m = check_pnpl_scenes(false, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad_args(who, "d_R, d_t, d_K or d_count is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.R = d_R; a.t = d_t; a.status = d_status; a.usable_mask = usable_mask;
    a.thresh = thresh; a.count = d_count;
    launch_slabs(cvxnl::score_kernel, n_hyp, cvxnl::BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("score_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_select(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                          int64_t n_lines, const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status,
                                          const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                          const double *d_line_3d, double thresh, double *d_out_R, double *d_out_t, int32_t *d_head, uint8_t *d_mask_pts,
                                          uint8_t *d_mask_lines, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_select";
    cvxnl::SelectArgs a;
    if (const char *m = check_pnpl_scenes(false, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (n_hyp < 1) return bad_args(who, "a scene needs at least one hypothesis");
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines))
        return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.thresh = thresh;
    a.out_R = d_out_R; a.out_t = d_out_t; a.head = d_head; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines;
    hipLaunchKernelGGL(cvxnl::select_kernel, dim3((unsigned)n_scenes), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_assemble_consensus(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                                      int64_t n_lines, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                                      const double *d_line_3d, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_K,
                                                      int32_t K_per_scene, double *d_B27, double *d_Q45, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_assemble_consensus";
    cvxnl::ConsensusArgs a;
    if (const char *m = check_pnpl_scenes(false, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_K || !d_B27 || !d_Q45 || !d_count || (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines)) return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines; a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxnl::assemble_consensus_kernel, dim3((unsigned)n_scenes), dim3(64), 0, (hipStream_t)stream, a);
    return launched("assemble_consensus_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_refit_update(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                                const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count,
                                                const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                                const double *d_line_2d, const double *d_line_3d, double thresh, double *d_R, double *d_t, int32_t *d_head,
                                                uint8_t *d_mask_pts, uint8_t *d_mask_lines, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_refit_update";
    cvxnl::RefitArgs a;
    if (const char *m = check_pnpl_scenes(false, n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_fit_R || !d_fit_t || !d_fit_status || !d_fit_count || !d_K || !d_R || !d_t || !d_head || (n_pts > 0 && !d_mask_pts) ||
        (n_lines > 0 && !d_mask_lines))
        return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status; a.fit_cnt = d_fit_count;
    a.thresh = thresh; a.io_R = d_R; a.io_t = d_t; a.head = d_head; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines;
    hipLaunchKernelGGL(cvxnl::refit_update_kernel, dim3((unsigned)n_scenes), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    return launched("refit_update_kernel launch");
}
