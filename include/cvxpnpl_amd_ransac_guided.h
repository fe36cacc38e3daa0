/*
 * cvxpnpl_amd_ransac_guided.h -- C ABI of guided RANSAC over many scenes: minimal sets drawn from the best-ranked correspondences first
 * (libcvxpnpl_amd_ransac_guided.so).
 *
 * A library of its own beside libcvxpnpl_amd_ransac.so and libcvxpnpl_amd_ransac_adaptive.so, whose scene layout it shares: d_scene_2d
 * [n_total][2], d_scene_3d [n_total][3] (float64), d_offsets [n_scenes + 1] int64 on the DEVICE, d_K [n_scenes][9] or NULL; every kernel
 * clamps a scene's slice to [0, n_total).  Its kernels are held against a resource table of their own
 * (tests/golden/ransac_guided_kernel_resources.json).
 *
 * Every correspondence carries a quality (a matcher's score; higher is better).  `rank` turns the qualities into d_order [n_total] int32:
 * scene f's slice is a permutation of 0 .. M_f - 1, indices within the scene, best first.  j comes before m when key_j > key_m, or
 * key_j == key_m and j < m; the key is the quality, a NaN taken as -infinity (equal qualities give the identity; +0 and -0 tie).
 *
 * Hypothesis h of a scene draws from a POOL of its n(h) best-ranked correspondences (cvxpnpl_ransac_guided_pool_host):
 *   h >= pool_full:  n(h) = M_f, and the draw is the one cvxpnpl_ransac_sample_scenes makes for (M_f, seed_f, h), used directly as
 *                    scene indices (d_order is not read): bit for bit the uniform sampler.  pool_full = 0 is the uniform sampler.
 *   h <  pool_full:  n(h) = min(n_T(h), 4 + h, M_f), n_T(h) the smallest n of 4 .. M_f with
 *                    pool_full * ((n/M) * ((n-1)/(M-1)) * ((n-2)/(M-2)) * ((n-3)/(M-3))) >= h + 1  (float64, in this order; M_f if none),
 *                    and the minimal set is d_order[beg_f + pick[j]], pick the draw for (n(h), seed_f, h).
 * The Philox counter of a draw is the hypothesis index within the scene, and n(h) depends on (h, M_f, pool_full) alone, so hypothesis h
 * of scene f is the same draw whether it comes from `sample` or from a round of `sample_active`.
 *
 * A scene of fewer than 4 correspondences, or an entry of d_order outside [0, M_f), gives the NaN hypothesis with d_idx = -1.  An entry
 * of d_active outside [0, n_scenes) is skipped: nothing is stored for it.
 *
 * rank, sample and sample_active are asynchronous on `stream` and return 0, -1 for null or inconsistent arguments (nothing is launched;
 * the message is cvxpnpl_ransac_guided_last_error() and names the argument) or -2 for a HIP error.  A zero-size call is a no-op returning
 * 0.  Their pointers are DEVICE pointers on the current device.  rank_host and pool_host touch no device.
 */
#ifndef CVXPNPL_AMD_RANSAC_GUIDED_H
#define CVXPNPL_AMD_RANSAC_GUIDED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The ranking: d_order [n_total] int32 from d_quality [n_total] float64.  max_corr: the largest M_f (a host number, it sizes the grid;
 * a longer scene is still ranked completely, only slower).  One lane per correspondence counts the records of its scene that come
 * before it: O(M_f^2) per scene, no atomics, every slot of a scene's slice written exactly once.  Correspondences outside every scene's
 * slice keep what d_order held.  n_scenes = 0, n_total = 0 or max_corr = 0: no-op.
 */
int cvxpnpl_ransac_guided_rank(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, int32_t max_corr, const double *d_quality,
                               int32_t *d_order, void *stream);

/*
 * n_hyp minimal sets per scene, hypothesis (f, h) being problem f * n_hyp + h: the outputs of cvxpnpl_ransac_sample_scenes.
 *   d_seeds [n_scenes] uint64
 *   d_order [n_total] int32 (may be NULL when pool_full = 0)
 *   d_K     [n_scenes][9] or NULL; given, every problem also gets d_K_hyp [n_scenes * n_hyp][9] = d_K[f]
 *   d_idx   [n_scenes * n_hyp][4] int32, indices within the scene (optional)
 *   d_pts_2d [n_scenes * n_hyp][4][2], d_pts_3d [n_scenes * n_hyp][4][3]
 * pool_full >= 0.  n_hyp = 0: no-op.
 */
int cvxpnpl_ransac_guided_sample(int64_t n_scenes, int32_t n_hyp, int32_t pool_full, const int64_t *d_offsets, int64_t n_total,
                                 const uint64_t *d_seeds, const int32_t *d_order, const double *d_scene_2d, const double *d_scene_3d,
                                 const double *d_K, int32_t *d_idx, double *d_pts_2d, double *d_pts_3d, double *d_K_hyp, void *stream);

/*
 * The minimal sets of a round of the adaptive call (include/cvxpnpl_amd_ransac_adaptive.h): entry a draws the hypotheses
 * hyp0 .. hyp0 + n_round - 1 of scene f = d_active[a] as problems a * n_round + h, exactly what `sample` draws for those indices.
 * 0 <= hyp0, hyp0 + n_round <= cap.  Outputs as cvxpnpl_ransac_adaptive_sample: [n_active * n_round] problems.
 * n_active = 0 or n_round = 0: no-op.
 */
int cvxpnpl_ransac_guided_sample_active(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                        int32_t cap, int32_t pool_full, const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds,
                                        const int32_t *d_order, const double *d_scene_2d, const double *d_scene_3d, const double *d_K,
                                        int32_t *d_idx, double *d_pts_2d, double *d_pts_3d, double *d_K_hyp, void *stream);

/*
 * The ranking on the host, by the comparator the kernel uses: offsets [n_scenes + 1], quality [n_total], order [n_total] are HOST
 * pointers; slices are clamped as on the device.  n_threads <= 0: one per hardware thread.  Returns 0 or -1.
 */
int cvxpnpl_ransac_guided_rank_host(int64_t n_scenes, const int64_t *offsets, int64_t n_total, const double *quality, int32_t *order,
                                    int32_t n_threads);

/*
 * The pool size n(h) on the host, by the function the kernels call.  -1 for h < 0, n_corr < 4 or pool_full < 0.
 */
int32_t cvxpnpl_ransac_guided_pool_host(int32_t h, int32_t n_corr, int32_t pool_full);

/* Message of the calling thread's last failed call ("" if none). */
const char *cvxpnpl_ransac_guided_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* CVXPNPL_AMD_RANSAC_GUIDED_H */
