/*
 * cvxpnpl_amd_ransac_pnpl_lo.h -- C ABI of local optimisation in adaptive RANSAC over scenes of points AND lines: at the end of every
 * round the running best pose of each scene still active is refitted on the points and lines within a threshold of it by the non-minimal
 * solver, and the inlier count of the refitted pose -- points plus lines, a line counting once -- drives the stopping rule
 * (libcvxpnpl_amd_ransac_pnpl_lo.so).
 *
 * A library of its own beside libcvxpnpl_amd_ransac_pnpl.so and libcvxpnpl_amd_ransac_pnpl_adaptive.so, whose scene layout and state it
 * shares: d_pts_2d [n_pts][2], d_pts_3d [n_pts][3], d_line_2d [n_lines][4] (u0 v0 u1 v1), d_line_3d [n_lines][6] (P0 P1) (float64),
 * d_pt_offsets and d_ln_offsets [n_scenes + 1] int64 on the DEVICE, d_K [9] or [n_scenes][9]; every kernel clamps both slices of a scene.
 * A round's arrays are COMPACT: entry a < n_active of d_active names scene f = d_active[a]; an entry outside [0, n_scenes) is skipped --
 * its rows stay untouched.  Sampling, the minimal solves, the round's own update and the compaction are the other libraries',
 * unchanged; the counter of the refits taken is zeroed by cvxpnpl_ransac_lo_init (cvxpnpl_amd_ransac_lo.h), which reads nothing of a
 * scene; the solve between the two kernels here is cvxpnpl_solve_cost_batch.  Its kernels are held against a resource table of their own
 * (tests/golden/ransac_pnpl_lo_kernel_resources.json).
 *
 * One LO step k of n, with widening w:  m_k = 1 + (w - 1)(n - 1 - k) / max(n - 1, 1)  (w in the first step, 1 in the last).
 *   assemble  the cost of the points that pass the point predicate of cvxpnpl_ransac_pnpl_score (depth > 0 and r^2 < tau^2) and of the
 *             lines that pass its line predicate (both end points in front of the camera and within tau pixels of the image line; a
 *             degenerate 2D line is never taken; a NaN compares false) at the scene's running pose with tau = thresh * m_k -- the caller
 *             passes the product
 *   solve     cvxpnpl_solve_cost_batch on the n_active costs
 *   update    the refitted pose, counted at thresh, is taken when its status is 0 or 2, it was fitted to at least four correspondences
 *             and it counts at least max(d_best[f], d_head[f][1]): the non-minimal fit wins a tie
 *
 * Every entry point but assemble_host is asynchronous on `stream` and returns 0, -1 for null or inconsistent arguments (nothing is
 * launched; the message is cvxpnpl_ransac_pnpl_lo_last_error() and names the argument) or -2 for a HIP error.  A call with n_scenes = 0
 * or n_active = 0 is a no-op returning 0.  All pointers but assemble_host's are DEVICE pointers on the current device.
 */
#ifndef CVXPNPL_AMD_RANSAC_PNPL_LO_H
#define CVXPNPL_AMD_RANSAC_PNPL_LO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The assembly of a step: d_B27 [n_active][27], d_Q45 [n_active][45] and d_count [n_active] of the points and lines of scene
 * f = d_active[a] that pass the predicates at (d_R, d_t)[f] -- the running poses, [n_scenes][9] and [n_scenes][3] -- under thresh_k.  No
 * mask is read or written.  The sums meet in a fixed order -- a lane's points, then its lines; the lanes of a wavefront; the four
 * wavefronts -- about the centre of the first three taken 3D records in the order "points, then lines": the result depends on the inputs
 * alone.  Fewer than three correspondences taken (or a singular system, or a singular K): NaN cost, with the count reported.
 */
int cvxpnpl_ransac_pnpl_lo_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, const int64_t *d_pt_offsets, int64_t n_pts,
                                    const int64_t *d_ln_offsets, int64_t n_lines, const double *d_pts_2d, const double *d_pts_3d,
                                    const double *d_line_2d, const double *d_line_3d, const double *d_R, const double *d_t, const double *d_K,
                                    int32_t K_per_scene, double thresh_k, double *d_B27, double *d_Q45, int32_t *d_count, void *stream);

/*
 * The update of a step: (d_fit_R, d_fit_t, d_fit_status, d_fit_count)[a] is the refit of entry a and the size of the set it was fitted
 * to.  When it is taken (above), d_io_R[f], d_io_t[f], d_head[f][0..1] = { status, inliers }, d_best[f] = inliers and the scene's
 * slices of d_mask_pts and d_mask_lines change together, d_head[f][2] keeps the index of the hypothesis that seeded the fit, and
 * d_lo_taken[f] goes up by one.  Taken or not, d_done[a] becomes 1 when d_hyp_used[f] >= cap or
 * d_hyp_used[f] >= N(d_best[f], P_f + L_f, confidence) (cvxpnpl_ransac_adaptive_needed_host); a flag that is 1 stays 1.
 * 0 < confidence < 1, cap >= 0.
 */
int cvxpnpl_ransac_pnpl_lo_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t cap, double confidence,
                                  const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                  const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count,
                                  const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                  const double *d_line_2d, const double *d_line_3d, double thresh, double *d_io_R, double *d_io_t,
                                  int32_t *d_head, int32_t *d_best, uint8_t *d_mask_pts, uint8_t *d_mask_lines, const int32_t *d_hyp_used,
                                  int32_t *d_lo_taken, int32_t *d_done, void *stream);

/*
 * cvxpnpl_ransac_pnpl_lo_assemble on HOST arrays, by the rules the kernel follows -- the same lanes, the same order of the sums --, on
 * n_threads host threads (<= 0: the hardware's concurrency).  Synchronous; no device is touched.
 */
int cvxpnpl_ransac_pnpl_lo_assemble_host(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *pt_offsets, int64_t n_pts,
                                         const int64_t *ln_offsets, int64_t n_lines, const double *pts_2d, const double *pts_3d,
                                         const double *line_2d, const double *line_3d, const double *R, const double *t, const double *K,
                                         int32_t K_per_scene, double thresh_k, double *B27, double *Q45, int32_t *count, int32_t n_threads);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_pnpl_lo_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_PNPL_LO_H */
