/*
 * cvxpnpl_amd_ransac_msac.h -- C ABI of MSAC scoring for RANSAC over many scenes: the hypothesis of a scene is selected by the truncated
 * quadratic cost of its reprojection residuals instead of by its inlier count (libcvxpnpl_amd_ransac_msac.so).
 *
 * A library of its own beside libcvxpnpl_amd_ransac.so and libcvxpnpl_amd_ransac_adaptive.so, whose scene layout, hypothesis layouts and
 * state it shares: d_scene_2d [n_total][2], d_scene_3d [n_total][3] (float64), d_offsets [n_scenes + 1] int64 on the DEVICE, d_K [9] or
 * [n_scenes][9]; every kernel clamps a scene's slice to [0, n_total).  Sampling, the minimal solves, the compaction of the active list,
 * the refits and the polish are the other libraries', unchanged.  Its kernels are held against a resource table of their own
 * (tests/golden/ransac_msac_kernel_resources.json).
 *
 * The gain of hypothesis h over its scene, with tau = thresh:
 *
 *     gain(h) = ( sum over the scene's points that pass the inlier predicate of (tau^2 - r^2) ) / tau^2
 *
 * r^2 = du^2 + dv^2 and the predicate (depth > 0 and r^2 < tau^2; a NaN compares false) are those of cvxpnpl_ransac_score_scenes, so
 * the count made beside the gain is that call's count.  gain lies in [0, count]; the highest gain is the lowest sum of min(r^2, tau^2),
 * a point behind the camera costing tau^2.  Every term is positive and a pose adds its terms serially in scene order: the gain of a
 * pose over a scene depends on the inputs alone -- the same bits from either scoring entry point and from launch to launch.  A
 * hypothesis that is not usable (its status outside usable_mask) gains 0.0 and counts 0.
 *
 * Two hypotheses are ordered by the higher gain, then the LOWER index; a gain that is not > 0 (negative, NaN) is read as 0.
 *
 * Every entry point but score_host is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is
 * launched; the message is cvxpnpl_ransac_msac_last_error()) or -2 for a HIP error.  A call with n_scenes = 0 or n_active = 0 is a no-op
 * returning 0.  All pointers but score_host's are DEVICE pointers on the current device.
 */
#ifndef CVXPNPL_AMD_RANSAC_MSAC_H
#define CVXPNPL_AMD_RANSAC_MSAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Scoring of a fixed budget: d_gain [n_scenes * n_hyp] float64 and d_count [n_scenes * n_hyp] int32 of hypothesis (f, h) =
 * (d_R, d_t, d_status)[f * n_hyp + h] over scene f.  d_status is optional (NULL: every hypothesis is usable); bit s of usable_mask set:
 * status s is scored.  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_msac_score_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_R,
                                     const double *d_t, const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene,
                                     const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_gain, int32_t *d_count,
                                     void *stream);

/*
 * Scoring of a round (cvxpnpl_ransac_adaptive_score's layout): d_gain, d_count [n_active * n_round];
 * (d_R, d_t, d_status)[a * n_round + h] is hypothesis h of entry a, scored over scene f = d_active[a].  An entry of d_active outside
 * [0, n_scenes) leaves its rows unwritten.  n_round = 0: no-op.
 */
int cvxpnpl_ransac_msac_score_active(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round, const int64_t *d_offsets,
                                     int64_t n_total, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                     const double *d_K, int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh,
                                     double *d_gain, int32_t *d_count, void *stream);

/*
 * Selection: per scene the hypothesis of the highest d_gain (the LOWEST index on an exact tie), laid out as
 * cvxpnpl_ransac_select_scenes lays it out: d_out_R [n_scenes][9], d_out_t [n_scenes][3], d_head [n_scenes][4] = { status of the pose,
 * inliers (the size of its mask), index within the scene, certified hypotheses }, d_mask [n_total]; and d_score [n_scenes] float64, the
 * winner's gain as the ordering read it, copied from d_gain.  The index is inside [0, n_hyp) whatever d_gain holds.  n_hyp >= 1.
 */
int cvxpnpl_ransac_msac_select_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_gain,
                                      const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                      const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                                      int32_t *d_head, uint8_t *d_mask, double *d_score, void *stream);

/*
 * Start of an adaptive call, after cvxpnpl_ransac_adaptive_init: d_best_gain[f] = -1 (below every gain).  n_scenes <= 2^31 - 1.
 */
int cvxpnpl_ransac_msac_init(int64_t n_scenes, double *d_best_gain, void *stream);

/*
 * The round's update, per active scene (cvxpnpl_ransac_adaptive_update's arguments, with d_gain beside d_count and d_best_gain beside
 * d_best): the arg-max of the round's gains replaces the scene's running best only when its gain is STRICTLY greater than
 * d_best_gain[f]; then d_out_R, d_out_t, d_head[f][0..2] = { status, inliers, hyp0 + index }, the scene's slice of d_mask,
 * d_best[f] = the d_count of that winner and d_best_gain[f] change together.  The round's certified hypotheses are added to
 * d_head[f][3], d_hyp_used[f] = hyp0 + n_round, and d_done[a] = 1 when the scene is finished:  hyp0 + n_round >= cap, or
 * hyp0 + n_round >= N(d_best[f], M_f, confidence) (cvxpnpl_ransac_adaptive_needed_host) -- the stopping rule reads the inlier COUNT of the
 * running winner.  n_round >= 1, 0 < confidence < 1.
 */
int cvxpnpl_ransac_msac_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round, int32_t cap,
                               double confidence, const int64_t *d_offsets, int64_t n_total, const double *d_gain, const int32_t *d_count,
                               const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                               const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                               int32_t *d_head, int32_t *d_best, double *d_best_gain, uint8_t *d_mask, int32_t *d_hyp_used, int32_t *d_done,
                               void *stream);

/*
 * cvxpnpl_ransac_msac_score_scenes on HOST arrays, by the functions the kernels call, on n_threads host threads (<= 0: the hardware's
 * concurrency).  Synchronous; no device is touched.
 */
int cvxpnpl_ransac_msac_score_host(int64_t n_scenes, int32_t n_hyp, const int64_t *offsets, int64_t n_total, const double *R, const double *t,
                                   const int32_t *status, uint32_t usable_mask, const double *K, int32_t K_per_scene, const double *scene_2d,
                                   const double *scene_3d, double thresh, double *gain, int32_t *count, int32_t n_threads);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_msac_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_MSAC_H */
