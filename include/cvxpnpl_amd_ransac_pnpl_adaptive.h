/*
 * cvxpnpl_amd_ransac_pnpl_adaptive.h -- C ABI of adaptive and guided RANSAC over point AND line correspondences, many scenes
 * (libcvxpnpl_amd_ransac_pnpl_adaptive.so).
 *
 * A library of its own beside libcvxpnpl_amd_ransac_pnpl.so, whose scene layout it shares: d_pts_2d [n_pts][2], d_pts_3d [n_pts][3],
 * d_line_2d [n_lines][2][2], d_line_3d [n_lines][2][3] (float64), d_pt_offsets and d_ln_offsets [n_scenes + 1] int64 on the DEVICE,
 * d_K [9] or [n_scenes][9]; every kernel clamps both slices of a scene.  A correspondence of scene f is an index c into the UNION of its
 * P_f points and L_f lines: c < P_f is point c, otherwise line c - P_f; M_f = P_f + L_f.  Its kernels are held against a resource table
 * of their own (tests/golden/ransac_pnpl_adaptive_kernel_resources.json).
 *
 * A call proceeds in rounds, as in cvxpnpl_amd_ransac_adaptive.h: d_active [n_active] int32 lists the scenes that still draw; round r
 * draws n_round further hypotheses for each of them, hypothesis h of entry a being problem a * n_round + h of the round's minimal solve
 * (the caller runs cvxpnpl_solve_cost_batch on those n_active * n_round costs between `sample_assemble` and `score`, on the same stream)
 * and hypothesis hyp0 + h of scene f = d_active[a].  What lasts over the rounds is indexed by the scene: d_out_R [n_scenes][9], d_out_t
 * [n_scenes][3], d_head [n_scenes][4], d_best [n_scenes], d_hyp_used [n_scenes], d_mask_pts [n_pts] and d_mask_lines [n_lines], laid
 * out as cvxpnpl_ransac_pnpl_select lays them out.  A scene that stops after u hypotheses holds what cvxpnpl_ransac_pnpl_select gives
 * over its first u hypotheses.  The start of a call, the compaction of the active list and the stopping rule on the host are
 * cvxpnpl_ransac_adaptive_init, _compact and _needed_host; the ranking of a quality is cvxpnpl_ransac_guided_rank over the union
 * offsets d_pt_offsets + d_ln_offsets.
 *
 * An entry of d_active outside [0, n_scenes) is skipped: nothing is stored for it.
 *
 * Every entry point is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is launched; the message
 * is cvxpnpl_ransac_pnpl_adaptive_last_error()) or -2 for a HIP error.  A call with n_scenes = 0 or n_active = 0 is a no-op returning
 * 0.  All pointers are DEVICE pointers on the current device.  n_scenes, n_active <= 2^31 - 1.
 */
#ifndef CVXPNPL_AMD_RANSAC_PNPL_ADAPTIVE_H
#define CVXPNPL_AMD_RANSAC_PNPL_ADAPTIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Minimal sets of a round and their costs: entry a draws the hypotheses hyp0 .. hyp0 + n_round - 1 of scene f = d_active[a] and
 * assembles each as cvxpnpl_ransac_pnpl_sample_assemble does.  0 <= hyp0, hyp0 + n_round <= cap, 0 <= pool_full.
 * Hypothesis hs of the scene draws four distinct ranks from the n(hs) = cvxpnpl_ransac_guided_pool_host(hs, M_f, pool_full) first; while
 * hs < pool_full its set is d_order[beg_f + rank], from pool_full on the rank IS the union index and d_order is not read.  pool_full = 0
 * is the uniform draw of cvxpnpl_ransac_pnpl_sample_assemble, bit for bit; the identity active list with hyp0 = 0 is its layout too.
 *   d_seeds [n_scenes] uint64
 *   d_order [n_pts + n_lines] int32: per scene, from beg_f = d_pt_offsets[f] + d_ln_offsets[f] on, union indices best first (NULL
 *           allowed when pool_full = 0).  An entry outside [0, M_f) is never followed: the hypotheses that read it get the NaN cost.
 *   d_idx   [n_active * n_round][4] int32, union indices within the scene (optional)
 *   d_Q45   [n_active * n_round][45], d_B27 [n_active * n_round][27]
 * M_f < 4, a singular K or a bad d_order entry: NaN cost and d_idx = -1.  n_round = 0: no-op.
 */
int cvxpnpl_ransac_pnpl_adaptive_sample_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                 int32_t cap, int32_t pool_full, const int64_t *d_pt_offsets, int64_t n_pts,
                                                 const int64_t *d_ln_offsets, int64_t n_lines, const uint64_t *d_seeds, const int32_t *d_order,
                                                 const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                                 const double *d_line_3d, const double *d_K, int32_t K_per_scene, int32_t *d_idx, double *d_Q45,
                                                 double *d_B27, void *stream);

/*
 * Consensus scoring of a round: d_count [n_active * n_round] int32, point plus line inliers by the predicates and the status rule of
 * cvxpnpl_ransac_pnpl_score; (d_R, d_t, d_status)[a * n_round + h] is hypothesis h of entry a.  n_round = 0: no-op.
 */
int cvxpnpl_ransac_pnpl_adaptive_score(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round,
                                       const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                       const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask, const double *d_K,
                                       int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                       const double *d_line_3d, double thresh, int32_t *d_count, void *stream);

/*
 * The round's update, per active scene: the arg-max of the round's counts (the LOWEST index on a tie) replaces the scene's running best
 * only when its count is STRICTLY greater than d_best[f]; then d_out_R, d_out_t, d_head[f][0..2] = { status, inliers, hyp0 + index },
 * d_best[f] and the scene's slices of d_mask_pts and d_mask_lines change together.  The round's certified hypotheses are added to
 * d_head[f][3], d_hyp_used[f] = hyp0 + n_round, and d_done[a] = 1 when the scene is finished:  hyp0 + n_round >= cap, or
 * hyp0 + n_round >= N(d_best[f], P_f + L_f, confidence) (cvxpnpl_ransac_adaptive_needed_host), compared in float64.
 * n_round >= 1, 0 < confidence < 1.
 */
int cvxpnpl_ransac_pnpl_adaptive_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round, int32_t cap,
                                        double confidence, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                        int64_t n_lines, const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status,
                                        const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                        const double *d_line_2d, const double *d_line_3d, double thresh, double *d_out_R, double *d_out_t,
                                        int32_t *d_head, int32_t *d_best, uint8_t *d_mask_pts, uint8_t *d_mask_lines, int32_t *d_hyp_used,
                                        int32_t *d_done, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_pnpl_adaptive_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_PNPL_ADAPTIVE_H */
