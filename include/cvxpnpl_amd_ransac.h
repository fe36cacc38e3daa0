/*
 * cvxpnpl_amd_ransac.h -- C ABI of RANSAC over many scenes of different sizes (libcvxpnpl_amd_ransac.so).
 *
 * A library of its own beside libcvxpnpl_amd.so, like the backward pass: the solves (include/cvxpnpl_amd.h) do not depend on it, and its
 * kernels are held against a resource table of their own (tests/golden/ransac_kernel_resources.json).  The entry points are the steps
 * AROUND the solves of a frame set; the caller runs cvxpnpl_solve_batch on the n_scenes * n_hyp minimal problems and
 * cvxpnpl_solve_cost_batch on the n_scenes refits in between, on the same stream.
 *
 * Layout.  The scenes are packed: d_scene_2d [n_total][2], d_scene_3d [n_total][3] (float64), scene f being the correspondences
 * d_offsets[f] .. d_offsets[f+1] - 1 of them; d_offsets [n_scenes + 1] is int64, on the DEVICE, non-decreasing, d_offsets[0] = 0,
 * d_offsets[n_scenes] = n_total.  Every kernel clamps a scene's slice to [0, n_total), so a wrong offset cannot become an access outside
 * the packed arrays.  Every scene has the same number n_hyp of hypotheses; hypothesis h of scene f is problem f * n_hyp + h.
 * d_K is [9] (K_per_scene = 0) or [n_scenes][9] (K_per_scene = 1), row-major.  All pointers are DEVICE pointers on the current device.
 *
 * Every entry point is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is launched; the message is
 * cvxpnpl_ransac_last_error()) or -2 for a HIP error.  A call with n_scenes = 0 is a no-op returning 0.
 */
#ifndef CVXPNPL_AMD_RANSAC_H
#define CVXPNPL_AMD_RANSAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Minimal sets: four distinct correspondences of its scene per hypothesis, gathered into the inputs of the minimal solve.  Scene f draws
 * exactly what cvxpnpl_sample_minimal_sets(n_hyp, M_f, scene f, k = 4, d_seeds[f]) draws: Philox4x32-10 keyed by the scene's seed, counter
 * (hypothesis index within the scene, 0xFFFFFFFE, 0), partial Fisher-Yates.
 *   d_seeds [n_scenes] uint64
 *   d_K     [n_scenes][9] or NULL; given, hypothesis (f, h) also gets d_K_hyp [n_scenes * n_hyp][9] = d_K[f] (the solver's per-problem K)
 *   d_idx   [n_scenes * n_hyp][4] int32, indices within the scene (optional)
 *   d_pts_2d [n_scenes * n_hyp][4][2], d_pts_3d [n_scenes * n_hyp][4][3]
 * A scene of fewer than four correspondences cannot be sampled: its hypotheses get NaN points (and index -1).  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_sample_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds,
                                 const double *d_scene_2d, const double *d_scene_3d, const double *d_K, int32_t *d_idx, double *d_pts_2d,
                                 double *d_pts_3d, double *d_K_hyp, void *stream);

/*
 * Consensus scoring: d_count [n_scenes * n_hyp] int32, the correspondences of scene f that hypothesis (f, h) = (d_R, d_t)[f * n_hyp + h]
 * explains (in front of the camera, reprojection error below thresh pixels).  d_status (optional) with usable_mask as in
 * cvxpnpl_score_hypotheses: a hypothesis whose status bit is not set, or whose pose is not finite, scores 0.  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_score_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_R, const double *d_t,
                                const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene, const double *d_scene_2d,
                                const double *d_scene_3d, double thresh, int32_t *d_count, void *stream);

/*
 * Selection, per scene what cvxpnpl_select_best does for one: the hypothesis of the highest count (the LOWEST index on a tie), its pose in
 * d_out_R [n_scenes][9] / d_out_t [n_scenes][3], its inlier mask in the scene's slice of d_mask [n_total] (uint8, 0 / 1), and
 * d_head [n_scenes][4] int32 = { status of the pose, inliers, index of the winner within the scene, certified hypotheses of the scene }.
 * n_hyp >= 1.
 */
int cvxpnpl_ransac_select_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const int32_t *d_count,
                                 const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                 const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                                 int32_t *d_head, uint8_t *d_mask, void *stream);

/*
 * Constraint assembly of every scene's consensus set (the correspondences with d_mask != 0), for cvxpnpl_solve_cost_batch:
 * d_B27 [n_scenes][27], d_Q45 [n_scenes][45], d_count [n_scenes] int32 (the size of each set).  One wavefront per scene, deterministic.
 * A set of fewer than three correspondences gives NaN for its scene.
 */
int cvxpnpl_ransac_assemble_consensus(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_scene_2d,
                                      const double *d_scene_3d, const uint8_t *d_mask, const double *d_K, int32_t K_per_scene, double *d_B27,
                                      double *d_Q45, int32_t *d_count, void *stream);

/*
 * Refit update, per scene the rule of cvxpnpl_refit_update: the refitted pose d_fit_R [n_scenes][9] / d_fit_t [n_scenes][3] is taken --
 * pose, status (d_head[f][0]), mask and count (d_head[f][1]) together, in place -- when d_fit_status[f] is 0 or 2, it was fitted to
 * d_fit_count[f] >= 4 correspondences and it keeps at least d_head[f][1] inliers; otherwise everything of the scene stays.
 */
int cvxpnpl_ransac_refit_update_scenes(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_fit_R, const double *d_fit_t,
                                       const int32_t *d_fit_status, const int32_t *d_fit_count, const double *d_K, int32_t K_per_scene,
                                       const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_R, double *d_t,
                                       int32_t *d_head, uint8_t *d_mask, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_H */
