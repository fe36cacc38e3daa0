/*
 * cvxpnpl_amd_ransac_adaptive.h -- C ABI of adaptive RANSAC over many scenes: a hypothesis budget per scene, solved in rounds
 * (libcvxpnpl_amd_ransac_adaptive.so).
 *
 * A library of its own beside libcvxpnpl_amd_ransac.so, whose scene layout it shares: d_scene_2d [n_total][2], d_scene_3d [n_total][3]
 * (float64), d_offsets [n_scenes + 1] int64 on the DEVICE, d_K [9] or [n_scenes][9]; every kernel clamps a scene's slice to [0, n_total).
 * Its kernels are held against a resource table of their own (tests/golden/ransac_adaptive_kernel_resources.json).
 *
 * A call proceeds in rounds.  d_active [n_active] int32 lists the scenes that still draw; round r draws n_round further hypotheses for
 * each of them, hypothesis h of entry a being problem a * n_round + h of the round's minimal solve (the caller runs cvxpnpl_solve_batch
 * on those n_active * n_round problems between `sample` and `score`, on the same stream) and hypothesis hyp0 + h of scene
 * f = d_active[a].  hyp0 is the same for every active scene, because an active scene has taken part in every earlier round.  What lasts
 * over the rounds is indexed by the scene: d_out_R [n_scenes][9], d_out_t [n_scenes][3], d_head [n_scenes][4], d_best [n_scenes],
 * d_hyp_used [n_scenes] and d_mask [n_total], laid out as cvxpnpl_ransac_select_scenes lays them out.  A scene that stops after u
 * hypotheses holds what cvxpnpl_ransac_select_scenes gives over its first u hypotheses.
 *
 * An entry of d_active outside [0, n_scenes) is skipped: nothing is stored for it, and the compaction drops it.
 *
 * Every entry point but needed_host is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is launched;
 * the message is cvxpnpl_ransac_adaptive_last_error()) or -2 for a HIP error.  A call with n_scenes = 0 or n_active = 0 is a no-op
 * returning 0.  All pointers are DEVICE pointers on the current device.
 */
#ifndef CVXPNPL_AMD_RANSAC_ADAPTIVE_H
#define CVXPNPL_AMD_RANSAC_ADAPTIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Start of a call: d_active[i] = i, d_n_active[0] = n_scenes, d_head[f] = { 3, -1, 0, 0 }, d_best[f] = -1, d_hyp_used[f] = 0.
 * n_scenes <= 2^31 - 1.
 */
int cvxpnpl_ransac_adaptive_init(int64_t n_scenes, int32_t *d_active, int32_t *d_n_active, int32_t *d_head, int32_t *d_best,
                                 int32_t *d_hyp_used, void *stream);

/*
 * Minimal sets of a round: entry a draws the hypotheses hyp0 .. hyp0 + n_round - 1 of scene f = d_active[a], exactly the draws
 * cvxpnpl_ransac_sample_scenes makes for those indices (the Philox counter is the index within the scene).  0 <= hyp0,
 * hyp0 + n_round <= cap.
 *   d_seeds [n_scenes] uint64
 *   d_K     [n_scenes][9] or NULL; given, problem (a, h) also gets d_K_hyp [n_active * n_round][9] = d_K[f]
 *   d_idx   [n_active * n_round][4] int32, indices within the scene (optional)
 *   d_pts_2d [n_active * n_round][4][2], d_pts_3d [n_active * n_round][4][3]
 * n_round = 0: no-op.
 */
int cvxpnpl_ransac_adaptive_sample(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round, int32_t cap,
                                   const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds, const double *d_scene_2d,
                                   const double *d_scene_3d, const double *d_K, int32_t *d_idx, double *d_pts_2d, double *d_pts_3d,
                                   double *d_K_hyp, void *stream);

/*
 * Consensus scoring of a round: d_count [n_active * n_round] int32, the predicate and the status rule of cvxpnpl_ransac_score_scenes;
 * (d_R, d_t, d_status)[a * n_round + h] is hypothesis h of entry a.  n_round = 0: no-op.
 */
int cvxpnpl_ransac_adaptive_score(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round, const int64_t *d_offsets,
                                  int64_t n_total, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                  const double *d_K, int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh,
                                  int32_t *d_count, void *stream);

/*
 * The round's update, per active scene: the arg-max of the round's counts (the LOWEST index on a tie) replaces the scene's running best
 * only when its count is STRICTLY greater than d_best[f]; then d_out_R, d_out_t, d_head[f][0..2] = { status, inliers, hyp0 + index },
 * d_best[f] and the scene's slice of d_mask change together.  The round's certified hypotheses are added to d_head[f][3],
 * d_hyp_used[f] = hyp0 + n_round, and d_done[a] = 1 when the scene is finished:  hyp0 + n_round >= cap, or
 * hyp0 + n_round >= N(d_best[f], M_f, confidence) (cvxpnpl_ransac_adaptive_needed_host), compared in float64.
 * n_round >= 1, 0 < confidence < 1.
 */
int cvxpnpl_ransac_adaptive_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round, int32_t cap,
                                   double confidence, const int64_t *d_offsets, int64_t n_total, const int32_t *d_count, const double *d_R,
                                   const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                   const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                                   int32_t *d_head, int32_t *d_best, uint8_t *d_mask, int32_t *d_hyp_used, int32_t *d_done, void *stream);

/*
 * Compaction: d_active_next = the entries of d_active whose d_done is 0, in order, and d_n_active_next[0] their number.  One workgroup,
 * no atomics: the same inputs give the same bits.  d_active_next must not be d_active.  n_active <= 2^31 - 1.
 */
int cvxpnpl_ransac_adaptive_compact(int64_t n_scenes, int64_t n_active, const int32_t *d_active, const int32_t *d_done,
                                    int32_t *d_active_next, int32_t *d_n_active_next, void *stream);

/*
 * The stopping rule on the host, by the function the update kernel calls:  N = log(1 - confidence) / log1p(-q),
 * q = prod_{j = 0..3} (inliers - j) / (n_corr - j);  inf for inliers < 4, 0 for inliers >= n_corr, NaN for a confidence outside (0, 1).
 * No device is touched.
 */
double cvxpnpl_ransac_adaptive_needed_host(int32_t inliers, int32_t n_corr, double confidence);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_adaptive_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_ADAPTIVE_H */
