/*
 * cvxpnpl_amd_ransac_pnpl.h -- C ABI of RANSAC over point AND line correspondences, many scenes of different sizes
 * (libcvxpnpl_amd_ransac_pnpl.so).
 *
 * The fourth library, beside the solver's (include/cvxpnpl_amd.h), the backward pass and the point-only RANSAC
 * (include/cvxpnpl_amd_ransac.h), none of which depends on it; its kernels are held against a resource table of their own
 * (tests/golden/ransac_pnpl_kernel_resources.json).  The entry points are the steps AROUND the solves of a frame set.  A minimal set is
 * four correspondences drawn from the union of a scene's points and lines, so it has one of five shapes (4+0 .. 0+4) and cannot go
 * through cvxpnpl_solve_batch, which takes one (n_p, n_l) per batch: the sampling step assembles each hypothesis' cost itself and the
 * caller runs cvxpnpl_solve_cost_batch on the n_scenes * n_hyp costs, and again on the n_scenes refits, on the same stream.
 *
 * Layout.  A scene set is two packed correspondence arrays with an offset array each:
 *   points  d_pts_2d  [n_pts][2],     d_pts_3d  [n_pts][3];       scene f holds the points d_pt_offsets[f] .. d_pt_offsets[f+1] - 1
 *   lines   d_line_2d [n_lines][2][2], d_line_3d [n_lines][2][3];  scene f holds the lines  d_ln_offsets[f] .. d_ln_offsets[f+1] - 1
 * (float64; a 2D line is two pixel samples ON the image line, a 3D line its two end points -- the layout of cvxpnpl_solve_batch).  Both
 * offset arrays are int64 [n_scenes + 1] on the DEVICE, non-decreasing, starting at 0 and ending at n_pts / n_lines.  Every kernel clamps
 * a scene's slices to [0, n_pts) and [0, n_lines), so a wrong offset cannot become an access outside the packed arrays.  Either array may
 * be empty (n_pts = 0 or n_lines = 0, pointers NULL), for the whole set or for single scenes.  Every scene has the same number n_hyp of
 * hypotheses; hypothesis h of scene f is problem f * n_hyp + h.  d_K is [9] (K_per_scene = 0) or [n_scenes][9] (K_per_scene = 1),
 * row-major.  All pointers are DEVICE pointers on the current device.
 *
 * The inlier predicates.  A point is an inlier of a pose as in cvxpnpl_ransac_score_scenes: in front of the camera and reprojected
 * within thresh pixels.  A line with 2D samples a, b and 3D end points P0, P1 is an inlier when both end points lie in front of the
 * camera (depth > 0) and both projected end points (u, v) lie within thresh pixels of the image line l = (a, 1) x (b, 1):
 *   |l . (u, v, 1)| / hypot(l_0, l_1) < thresh.
 * A pose that is not finite, or a degenerate 2D line (a = b), compares false.  An inlier COUNT is points plus lines; a line counts once.
 *
 * Every entry point is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is launched; the message is
 * cvxpnpl_ransac_pnpl_last_error()) or -2 for a HIP error.  A call with n_scenes = 0 is a no-op returning 0.
 */
#ifndef CVXPNPL_AMD_RANSAC_PNPL_H
#define CVXPNPL_AMD_RANSAC_PNPL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Minimal sets and their costs.  Hypothesis (f, h) draws four distinct indices of 0 .. M_f - 1, M_f = P_f + L_f, exactly as
 * cvxpnpl_ransac_sample_scenes does over M_f (Philox4x32-10 keyed by d_seeds[f], counter (h, 0, 0xFFFFFFFE, 0), partial Fisher-Yates):
 * index c < P_f is point c of the scene, otherwise line c - P_f.  With L_f = 0 a scene draws what cvxpnpl_ransac_sample_scenes draws.
 * The set -- its points in draw order, then its lines in draw order -- is assembled as cvxpnpl_assemble_batch assembles it:
 *   d_Q45 [n_scenes * n_hyp][45], d_B27 [n_scenes * n_hyp][27]   the inputs of cvxpnpl_solve_cost_batch
 *   d_idx [n_scenes * n_hyp][4] int32   the drawn indices (optional)
 * A scene of fewer than four correspondences, or a singular K: NaN cost and index -1.  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_pnpl_sample_assemble(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                        int64_t n_lines, const uint64_t *d_seeds, const double *d_pts_2d, const double *d_pts_3d,
                                        const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_scene, int32_t *d_idx,
                                        double *d_Q45, double *d_B27, void *stream);

/*
 * Consensus scoring: d_count [n_scenes * n_hyp] int32, the points plus the lines of scene f that hypothesis (f, h) =
 * (d_R, d_t)[f * n_hyp + h] explains.  d_status (optional) with usable_mask as in cvxpnpl_score_hypotheses: a hypothesis whose status bit
 * is not set, or whose pose is not finite, scores 0.  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_pnpl_score(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                              int64_t n_lines, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                              const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                              const double *d_line_3d, double thresh, int32_t *d_count, void *stream);

/*
 * Selection: per scene the hypothesis of the highest count (the LOWEST index on a tie), its pose in d_out_R [n_scenes][9] /
 * d_out_t [n_scenes][3], its inlier masks in the scene's slices of d_mask_pts [n_pts] and d_mask_lines [n_lines] (uint8, 0 / 1), and
 * d_head [n_scenes][4] int32 = { status of the pose, inliers (points + lines), index of the winner within the scene, certified
 * hypotheses of the scene }.  n_hyp >= 1.
 */
int cvxpnpl_ransac_pnpl_select(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                               int64_t n_lines, const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status,
                               const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                               const double *d_line_3d, double thresh, double *d_out_R, double *d_out_t, int32_t *d_head, uint8_t *d_mask_pts,
                               uint8_t *d_mask_lines, void *stream);

/*
 * Constraint assembly of every scene's consensus set (the points with d_mask_pts != 0, then the lines with d_mask_lines != 0), for
 * cvxpnpl_solve_cost_batch: d_B27 [n_scenes][27], d_Q45 [n_scenes][45], d_count [n_scenes] int32 (points + lines taken).  One wavefront
 * per scene, deterministic.  A set of fewer than three correspondences, a singular N^T N or a singular K gives NaN for its scene only.
 */
int cvxpnpl_ransac_pnpl_assemble_consensus(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                           int64_t n_lines, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                           const double *d_line_3d, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_K,
                                           int32_t K_per_scene, double *d_B27, double *d_Q45, int32_t *d_count, void *stream);

/*
 * Refit update, the rule of cvxpnpl_ransac_refit_update_scenes: the refitted pose d_fit_R [n_scenes][9] / d_fit_t [n_scenes][3] is taken
 * -- pose, status (d_head[f][0]), both masks and count (d_head[f][1]) together, in place -- when d_fit_status[f] is 0 or 2, it was fitted
 * to d_fit_count[f] >= 4 correspondences and it keeps at least d_head[f][1] inliers; otherwise everything of the scene stays.
 */
int cvxpnpl_ransac_pnpl_refit_update(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                     const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count,
                                     const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                     const double *d_line_2d, const double *d_line_3d, double thresh, double *d_R, double *d_t, int32_t *d_head,
                                     uint8_t *d_mask_pts, uint8_t *d_mask_lines, void *stream);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_pnpl_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_PNPL_H */
