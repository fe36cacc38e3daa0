// ransac_pnpl_adaptive_hip.hip -- entry points of adaptive and guided RANSAC over points and lines
// (include/cvxpnpl_amd_ransac_pnpl_adaptive.h), built as libcvxpnpl_amd_ransac_pnpl_adaptive.so.  The kernels are
// ransac_pnpl_adaptive_kernel.h, the stopping rule ransac_adaptive_core.h, the pool rule ransac_guided_core.h, the shared checks and the
// slab launch ransac_entry.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_pnpl_adaptive.h"
#include "ransac_entry.h"
#include "ransac_pnpl_adaptive_kernel.h"

using namespace cvxne;

extern "C" const char *cvxpnpl_ransac_pnpl_adaptive_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_pnpl_adaptive_sample_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                            int32_t cap, int32_t pool_full, const int64_t *d_pt_offsets, int64_t n_pts,
                                                            const int64_t *d_ln_offsets, int64_t n_lines, const uint64_t *d_seeds,
                                                            const int32_t *d_order, const double *d_pts_2d, const double *d_pts_3d,
                                                            const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_scene,
                                                            int32_t *d_idx, double *d_Q45, double *d_B27, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_sample_assemble";
    cvxnla::SampleArgs a;
    if (const char *m = check_pnpl_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad_args(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad_args(who, m);
    if (pool_full < 0) return bad_args(who, "negative pool_full");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_seeds || !d_K || !d_Q45 || !d_B27) return bad_args(who, "d_seeds, d_K, d_Q45 or d_B27 is null");
    if (pool_full > 0 && !d_order) return bad_args(who, "d_order is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.hyp0 = hyp0; a.n_round = n_round; a.pool_full = pool_full;
    a.active = d_active; a.seed = d_seeds; a.order = d_order; a.idx = d_idx; a.Q45 = d_Q45; a.B27 = d_B27;
    launch_slabs(cvxnla::sample_assemble_active_kernel, n_round, cvxnla::BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("sample_assemble_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_adaptive_score(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round,
                                                  const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                                  const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                                  const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                                  const double *d_line_2d, const double *d_line_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_score";
    cvxnla::ScoreArgs a;
    if (const char *m = check_pnpl_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad_args(who, m);
    if (n_round < 0) return bad_args(who, "negative n_round");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad_args(who, "d_R, d_t, d_K or d_count is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.n_round = n_round; a.active = d_active; a.R = d_R; a.t = d_t;
    a.status = d_status; a.usable_mask = usable_mask; a.thresh = thresh; a.count = d_count;
    launch_slabs(cvxnla::score_pnpl_active_kernel, n_round, cvxnla::BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("score_pnpl_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_adaptive_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                   int32_t cap, double confidence, const int64_t *d_pt_offsets, int64_t n_pts,
                                                   const int64_t *d_ln_offsets, int64_t n_lines, const int32_t *d_count, const double *d_R,
                                                   const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                                   const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                                   double thresh, double *d_out_R, double *d_out_t, int32_t *d_head, int32_t *d_best,
                                                   uint8_t *d_mask_pts, uint8_t *d_mask_lines, int32_t *d_hyp_used, int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_update";
    cvxnla::UpdateArgs a;
    if (const char *m = check_pnpl_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad_args(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad_args(who, m);
    if (cvxna::bad_confidence(confidence)) return bad_args(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (n_round < 1) return bad_args(who, "a round needs at least one hypothesis");
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || !d_best || !d_hyp_used || !d_done ||
        (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines))
        return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.hyp0 = hyp0; a.n_round = n_round; a.cap = cap; a.confidence = confidence;
    a.active = d_active; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t;
    a.head = d_head; a.best = d_best; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines; a.hyp_used = d_hyp_used; a.done = d_done;
    hipLaunchKernelGGL(cvxnla::update_pnpl_active_kernel, dim3((unsigned)n_active), dim3(cvxnla::BLOCK), 0, (hipStream_t)stream, a);
    return launched("update_pnpl_active_kernel launch");
}
