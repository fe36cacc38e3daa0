// ransac_adaptive_hip.hip -- entry points of adaptive RANSAC over many scenes (include/cvxpnpl_amd_ransac_adaptive.h), built as
// libcvxpnpl_amd_ransac_adaptive.so.  The kernels are ransac_adaptive_kernel.h, the stopping rule ransac_adaptive_core.h, the shared
// checks and the slab launch ransac_entry.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_adaptive.h"
#include "ransac_adaptive_kernel.h"
#include "ransac_entry.h"

using namespace cvxne;

extern "C" const char *cvxpnpl_ransac_adaptive_last_error(void) { return err_buf(); }

extern "C" double cvxpnpl_ransac_adaptive_needed_host(int32_t inliers, int32_t n_corr, double confidence)
{
    if (cvxna::bad_confidence(confidence)) return NAN;
    return cvxna::hyp_needed(inliers, n_corr, confidence);
}

extern "C" int cvxpnpl_ransac_adaptive_init(int64_t n_scenes, int32_t *d_active, int32_t *d_n_active, int32_t *d_head, int32_t *d_best,
                                            int32_t *d_hyp_used, void *stream)
{
    const char *who = "cvxpnpl_ransac_adaptive_init";
    if (const char *m = check_sizes(true, n_scenes, 0, 0)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (!d_active || !d_n_active || !d_head || !d_best || !d_hyp_used) return bad_args(who, "a null pointer");
    cvxna::InitArgs a;
    a.n_scenes = n_scenes; a.active = d_active; a.n_active = d_n_active; a.head = d_head; a.best = d_best; a.hyp_used = d_hyp_used;
    hipLaunchKernelGGL(cvxna::adaptive_init_kernel, dim3(blocks_for(n_scenes, cvxna::SCENE_BLOCK)), dim3(cvxna::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("adaptive_init_kernel launch");
}

extern "C" int cvxpnpl_ransac_adaptive_sample(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                              int32_t cap, const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds,
                                              const double *d_scene_2d, const double *d_scene_3d, const double *d_K, int32_t *d_idx,
                                              double *d_pts_2d, double *d_pts_3d, double *d_K_hyp, void *stream)
{
    const char *who = "cvxpnpl_ransac_adaptive_sample";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad_args(who, m);
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_seeds || !d_pts_2d || !d_pts_3d) return bad_args(who, "d_seeds, d_pts_2d or d_pts_3d is null");
    if ((d_K == nullptr) != (d_K_hyp == nullptr)) return bad_args(who, "d_K and d_K_hyp go together");
    cvxna::SampleActiveArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.hyp0 = hyp0; a.n_round = n_round; a.active = d_active; a.off = d_offsets;
    a.seed = d_seeds; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.K = d_K; a.idx = d_idx; a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.Kh = d_K_hyp;
    launch_slabs(cvxna::sample_active_kernel, n_round, cvxna::SCENE_BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("sample_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_adaptive_score(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round,
                                             const int64_t *d_offsets, int64_t n_total, const double *d_R, const double *d_t,
                                             const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene,
                                             const double *d_scene_2d, const double *d_scene_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_adaptive_score";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_round < 0) return bad_args(who, "negative n_round");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad_args(who, "d_R, d_t, d_K or d_count is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxna::ScoreActiveArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.n_round = n_round; a.active = d_active; a.off = d_offsets; a.R = d_R;
    a.t = d_t; a.status = d_status; a.usable_mask = usable_mask; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d;
    a.thresh = thresh; a.count = d_count;
    launch_slabs(cvxna::score_active_kernel, n_round, cvxna::SCENE_BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("score_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_adaptive_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                              int32_t cap, double confidence, const int64_t *d_offsets, int64_t n_total, const int32_t *d_count,
                                              const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K,
                                              int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh,
                                              double *d_out_R, double *d_out_t, int32_t *d_head, int32_t *d_best, uint8_t *d_mask,
                                              int32_t *d_hyp_used, int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_adaptive_update";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad_args(who, m);
    if (cvxna::bad_confidence(confidence)) return bad_args(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (n_round < 1) return bad_args(who, "a round needs at least one hypothesis");
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || !d_best || !d_hyp_used || !d_done ||
        (n_total > 0 && !d_mask))
        return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxna::RoundUpdateArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.hyp0 = hyp0; a.n_round = n_round; a.cap = cap; a.confidence = confidence;
    a.active = d_active; a.off = d_offsets; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.K = d_K; a.K_per_scene = K_per_scene;
    a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t; a.head = d_head; a.best = d_best;
    a.mask = d_mask; a.hyp_used = d_hyp_used; a.done = d_done;
    hipLaunchKernelGGL(cvxna::round_update_kernel, dim3((unsigned)n_active), dim3(cvxna::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("round_update_kernel launch");
}

extern "C" int cvxpnpl_ransac_adaptive_compact(int64_t n_scenes, int64_t n_active, const int32_t *d_active, const int32_t *d_done,
                                               int32_t *d_active_next, int32_t *d_n_active_next, void *stream)
{
    const char *who = "cvxpnpl_ransac_adaptive_compact";
    if (const char *m = check_sizes(true, n_scenes, n_active, 0)) return bad_args(who, m);
    if (n_scenes == 0 || n_active == 0) return 0;
    if (!d_active || !d_done || !d_active_next || !d_n_active_next) return bad_args(who, "a null pointer");
    if (d_active_next == d_active) return bad_args(who, "d_active_next must not be d_active");
    cvxna::CompactArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.active = d_active; a.done = d_done; a.active_next = d_active_next; a.n_active_next = d_n_active_next;
    hipLaunchKernelGGL(cvxna::compact_active_kernel, dim3(1), dim3(cvxna::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("compact_active_kernel launch");
}
