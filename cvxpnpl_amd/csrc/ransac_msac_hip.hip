// ransac_msac_hip.hip -- entry points of MSAC scoring for RANSAC over many scenes (include/cvxpnpl_amd_ransac_msac.h), built as
// libcvxpnpl_amd_ransac_msac.so.  The kernels are ransac_msac_kernel.h, the arithmetic ransac_msac_core.h, the shared checks and the slab
// launch ransac_entry.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_msac.h"
#include "host_pool.h"
#include "ransac_entry.h"
#include "ransac_msac_kernel.h"

using namespace cvxne;

extern "C" const char *cvxpnpl_ransac_msac_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_msac_score_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_R,
                                                const double *d_t, const int32_t *d_status, uint32_t usable_mask, const double *d_K,
                                                int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh,
                                                double *d_gain, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_msac_score_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (int rc = null_among(who, {{"d_R", d_R}, {"d_t", d_t}, {"d_K", d_K}, {"d_gain", d_gain}, {"d_count", d_count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxnm::ScoreScenesMsacArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.R = d_R; a.t = d_t; a.status = d_status;
    a.usable_mask = usable_mask; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.gain = d_gain;
    a.count = d_count;
    launch_slabs(cvxnm::score_scenes_msac_kernel, n_hyp, cvxnm::SCENE_BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("score_scenes_msac_kernel launch");
}

extern "C" int cvxpnpl_ransac_msac_score_active(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round,
                                                const int64_t *d_offsets, int64_t n_total, const double *d_R, const double *d_t,
                                                const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene,
                                                const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_gain,
                                                int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_msac_score_active";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_round < 0) return bad_args(who, "negative n_round");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (int rc = null_among(who, {{"d_R", d_R}, {"d_t", d_t}, {"d_K", d_K}, {"d_gain", d_gain}, {"d_count", d_count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxnm::ScoreActiveMsacArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.n_round = n_round; a.active = d_active; a.off = d_offsets; a.R = d_R;
    a.t = d_t; a.status = d_status; a.usable_mask = usable_mask; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d;
    a.thresh = thresh; a.gain = d_gain; a.count = d_count;
    launch_slabs(cvxnm::score_active_msac_kernel, n_round, cvxnm::SCENE_BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("score_active_msac_kernel launch");
}

extern "C" int cvxpnpl_ransac_msac_select_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_gain,
                                                 const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K,
                                                 int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh,
                                                 double *d_out_R, double *d_out_t, int32_t *d_head, uint8_t *d_mask, double *d_score, void *stream)
{
    const char *who = "cvxpnpl_ransac_msac_select_scenes";
    if (const char *m = check_scenes(false, n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (n_hyp < 1) return bad_args(who, "a scene needs at least one hypothesis");
    if (const char *m = check_one_launch(n_scenes)) return bad_args(who, m);
    if (int rc = null_among(who, {{"d_gain", d_gain}, {"d_R", d_R}, {"d_t", d_t}, {"d_status", d_status}, {"d_K", d_K}, {"d_out_R", d_out_R},
                                  {"d_out_t", d_out_t}, {"d_head", d_head}, {"d_score", d_score}}))
        return rc;
    if (n_total > 0 && !d_mask) return bad_args(who, "d_mask is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxnm::SelectScenesMsacArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.gain = d_gain; a.R = d_R; a.t = d_t; a.status = d_status;
    a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t;
    a.head = d_head; a.mask = d_mask; a.score = d_score;
    hipLaunchKernelGGL(cvxnm::select_scenes_msac_kernel, dim3((unsigned)n_scenes), dim3(cvxnm::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_scenes_msac_kernel launch");
}

extern "C" int cvxpnpl_ransac_msac_init(int64_t n_scenes, double *d_best_gain, void *stream)
{
    const char *who = "cvxpnpl_ransac_msac_init";
    if (const char *m = check_sizes(true, n_scenes, 0, 0)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (!d_best_gain) return bad_args(who, "d_best_gain is null");
    cvxnm::InitMsacArgs a;
    a.n_scenes = n_scenes; a.best_gain = d_best_gain;
    hipLaunchKernelGGL(cvxnm::msac_init_kernel, dim3(blocks_for(n_scenes, cvxnm::SCENE_BLOCK)), dim3(cvxnm::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("msac_init_kernel launch");
}

extern "C" int cvxpnpl_ransac_msac_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round, int32_t cap,
                                          double confidence, const int64_t *d_offsets, int64_t n_total, const double *d_gain,
                                          const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K,
                                          int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R,
                                          double *d_out_t, int32_t *d_head, int32_t *d_best, double *d_best_gain, uint8_t *d_mask,
                                          int32_t *d_hyp_used, int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_msac_update";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad_args(who, m);
    if (cvxna::bad_confidence(confidence)) return bad_args(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (n_round < 1) return bad_args(who, "a round needs at least one hypothesis");
    if (int rc = null_among(who, {{"d_gain", d_gain}, {"d_count", d_count}, {"d_R", d_R}, {"d_t", d_t}, {"d_status", d_status}, {"d_K", d_K},
                                  {"d_out_R", d_out_R}, {"d_out_t", d_out_t}, {"d_head", d_head}, {"d_best", d_best}, {"d_best_gain", d_best_gain},
                                  {"d_hyp_used", d_hyp_used}, {"d_done", d_done}}))
        return rc;
    if (n_total > 0 && !d_mask) return bad_args(who, "d_mask is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxnm::RoundUpdateMsacArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.hyp0 = hyp0; a.n_round = n_round; a.cap = cap; a.confidence = confidence;
    a.active = d_active; a.off = d_offsets; a.gain = d_gain; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.K = d_K;
    a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t; a.head = d_head;
    a.best = d_best; a.best_gain = d_best_gain; a.mask = d_mask; a.hyp_used = d_hyp_used; a.done = d_done;
    hipLaunchKernelGGL(cvxnm::round_update_msac_kernel, dim3((unsigned)n_active), dim3(cvxnm::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("round_update_msac_kernel launch");
}

extern "C" int cvxpnpl_ransac_msac_score_host(int64_t n_scenes, int32_t n_hyp, const int64_t *offsets, int64_t n_total, const double *R,
                                              const double *t, const int32_t *status, uint32_t usable_mask, const double *K, int32_t K_per_scene,
                                              const double *scene_2d, const double *scene_3d, double thresh, double *gain, int32_t *count,
                                              int32_t n_threads)
{
    const char *who = "cvxpnpl_ransac_msac_score_host";
    if (const char *m = check_sizes(false, n_scenes, 0, n_total)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!offsets) return bad_args(who, "offsets is null");
    if (n_total > 0 && (!scene_2d || !scene_3d)) return bad_args(who, "scene_2d or scene_3d is null");
    if (int rc = null_among(who, {{"R", R}, {"t", t}, {"K", K}, {"gain", gain}, {"count", count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    const double th2 = thresh * thresh;
    cvxh::for_chunks(n_scenes * n_hyp, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t g = lo; g < hi; ++g) { // the kernel's lane (f, h)
            const int64_t f = g / n_hyp;
            const cvxn::Slice sl = cvxn::scene_slice(offsets, f, n_total);
            const double *s2 = scene_2d + sl.beg * 2, *s3 = scene_3d + sl.beg * 3;
            cvxnm::Cam cam;
            cvxnm::cam_load(R + g * 9, t + g * 3, K + (K_per_scene ? f * 9 : 0), cam);
            const bool usable = cvxnm::hypothesis_usable(true, status, g, usable_mask);
            cvxnm::Sum acc{0.0, 0};
            for (int64_t m = 0; m < sl.n; ++m) // serially in scene order
                cvxnm::sum_add(acc, usable, cvxnm::point_gain(cam, s3[m * 3], s3[m * 3 + 1], s3[m * 3 + 2], s2[m * 2], s2[m * 2 + 1], th2));
            gain[g] = cvxnm::sum_gain(acc, th2);
            count[g] = acc.n;
        }
    });
    return 0;
}
