// ransac_hip.hip -- entry points of RANSAC over many scenes (include/cvxpnpl_amd_ransac.h), built as libcvxpnpl_amd_ransac.so.
// The kernels are ransac_kernel.h, the shared checks and the slab launch ransac_entry.h.  Every entry point checks its arguments before
// it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac.h"
#include "ransac_entry.h"
#include "ransac_kernel.h"

using namespace cvxne;

extern "C" const char *cvxpnpl_ransac_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_sample_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds,
                                            const double *d_scene_2d, const double *d_scene_3d, const double *d_K, int32_t *d_idx, double *d_pts_2d,
                                            double *d_pts_3d, double *d_K_hyp, void *stream)
{
    const char *who = "cvxpnpl_ransac_sample_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_seeds || !d_pts_2d || !d_pts_3d) return bad_args(who, "d_seeds, d_pts_2d or d_pts_3d is null");
    if ((d_K == nullptr) != (d_K_hyp == nullptr)) return bad_args(who, "d_K and d_K_hyp go together");
    cvxn::SampleScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.seed = d_seeds; a.s2 = d_scene_2d; a.s3 = d_scene_3d;
    a.K = d_K; a.idx = d_idx; a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.Kh = d_K_hyp;
    launch_slabs(cvxn::sample_scenes_kernel, n_hyp, cvxn::SCENE_BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("sample_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_score_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_R,
                                           const double *d_t, const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene,
                                           const double *d_scene_2d, const double *d_scene_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_score_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad_args(who, "d_R, d_t, d_K or d_count is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxn::ScoreScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.R = d_R; a.t = d_t; a.status = d_status;
    a.usable_mask = usable_mask; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.count = d_count;
    launch_slabs(cvxn::score_scenes_kernel, n_hyp, cvxn::SCENE_BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("score_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_select_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const int32_t *d_count,
                                            const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                            const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                                            int32_t *d_head, uint8_t *d_mask, void *stream)
{
    const char *who = "cvxpnpl_ransac_select_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (n_hyp < 1) return bad_args(who, "a scene needs at least one hypothesis");
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || (n_total > 0 && !d_mask)) return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxn::SelectScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status;
    a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t;
    a.head = d_head; a.mask = d_mask;
    hipLaunchKernelGGL(cvxn::select_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_assemble_consensus(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_scene_2d,
                                                 const double *d_scene_3d, const uint8_t *d_mask, const double *d_K, int32_t K_per_scene,
                                                 double *d_B27, double *d_Q45, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_assemble_consensus";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_K || !d_B27 || !d_Q45 || !d_count || (n_total > 0 && !d_mask)) return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    cvxn::ConsensusArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.off = d_offsets; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.mask = d_mask; a.K = d_K;
    a.K_per_scene = K_per_scene; a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxn::assemble_consensus_kernel, dim3((unsigned)n_scenes), dim3(64), 0, (hipStream_t)stream, a);
    return launched("assemble_consensus_kernel launch");
}

extern "C" int cvxpnpl_ransac_refit_update_scenes(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_fit_R,
                                                  const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count, const double *d_K,
                                                  int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_R,
                                                  double *d_t, int32_t *d_head, uint8_t *d_mask, void *stream)
{
    const char *who = "cvxpnpl_ransac_refit_update_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (!d_fit_R || !d_fit_t || !d_fit_status || !d_fit_count || !d_K || !d_R || !d_t || !d_head || (n_total > 0 && !d_mask)) return bad_args(who, "a null pointer");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxn::RefitScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.off = d_offsets; a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status;
    a.fit_cnt = d_fit_count; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.io_R = d_R;
    a.io_t = d_t; a.head = d_head; a.mask = d_mask;
    hipLaunchKernelGGL(cvxn::refit_update_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("refit_update_scenes_kernel launch");
}
