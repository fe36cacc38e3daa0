// ransac_lo_core.h -- the rules of local optimisation in adaptive RANSAC (include/cvxpnpl_amd_ransac_lo.h), ONE
// statement of them for the device (lo_assemble_active_kernel, lo_update_active_kernel) and the host (cvxpnpl_ransac_lo_assemble_host):
// which correspondences a step takes, which lane adds which correspondence, and when a refitted pose is taken.  The centre of the Gram
// sums, the order in which the partial sums meet, the finish and the NaN rule are ransac_assemble_core.h.
//
// The assembly of one active entry, by LANES = 256 lanes in four wavefronts:
//   taken(m)  = the inlier predicate of cvxn::is_inlier at the scene's running pose, threshold th2 = (thresh * m_k)^2
//   centre    = cvxas::centre of the first three taken correspondences in scene order
//   lane l    adds the taken correspondences m = l, l + 256, l + 512, ... in that order           (lane_sums)
//   a wave, the entry: cvxas::wave_butterfly and cvxas::waves_total
// so the 60 sums depend on the inputs alone.  On the device the camera and the predicate ARE cvxn::camera_load and cvxn::is_inlier; those
// are device-only, so the host build restates them expression by expression (as ransac_msac_core.h does).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_adaptive_core.h"
#include "ransac_assemble_core.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxnlo {

using cvxas::GRAM;
using cvxas::LANES;  // lanes of an assembly: the family's workgroup
using cvxas::WAVES;

// ---- the camera of a pose and the predicate
__host__ __device__ inline void camera(const double *Rp, const double *tp, const double *Kp, cvxn::Camera &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    cvxn::camera_load(Rp, tp, Kp, c);
#else
    double R[9], t[3], K[9];
    for (int i = 0; i < 9; ++i) { R[i] = Rp[i]; K[i] = Kp[i]; }
    for (int i = 0; i < 3; ++i) t[i] = tp[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) c.M[i * 4 + j] = K[i * 3] * R[j] + K[i * 3 + 1] * R[3 + j] + K[i * 3 + 2] * R[6 + j];
        c.M[i * 4 + 3] = K[i * 3] * t[0] + K[i * 3 + 1] * t[1] + K[i * 3 + 2] * t[2];
    }
    c.r2[0] = R[6]; c.r2[1] = R[7]; c.r2[2] = R[8]; c.t2 = t[2];
#endif
}
__host__ __device__ inline bool taken(const cvxn::Camera &c, const double *s2, const double *s3, int64_t m, double th2)
{
    const double X = s3[3 * m], Y = s3[3 * m + 1], Z = s3[3 * m + 2], x = s2[2 * m], y = s2[2 * m + 1];
#if defined(__HIP_DEVICE_COMPILE__)
    return cvxn::is_inlier(c, X, Y, Z, x, y, th2);
#else
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double du = u / w - x, dv = v / w - y;
    return depth > 0.0 && (du * du + dv * dv < th2);
#endif
}

// ---- lane l of an assembly: the Gram sums of the taken correspondences l, l + LANES, ... about the centre c; returns their number
__host__ __device__ inline int lane_sums(int l, int n, const double *s2, const double *s3, const cvxn::Camera &cam, double th2, const double *Ki,
                                         const double *c, cvx::Gram &g)
{
    cvx::gram_zero(g);
    int cnt = 0;
    for (int m = l; m < n; m += LANES) {
        if (!taken(cam, s2, s3, m, th2)) continue;
        cvx::gram_add_point(g, Ki, s2[2 * m], s2[2 * m + 1], s3[3 * m] - c[0], s3[3 * m + 1] - c[1], s3[3 * m + 2] - c[2]);
        ++cnt;
    }
    return cnt;
}

// ---- the update: a refitted pose of status st, fitted to fit_cnt correspondences and counting n_new inliers at thresh, is TAKEN when it
// is usable and holds at least the running best -- the rule of cvxn::refit_update_scenes_kernel: the non-minimal fit wins a tie.
__host__ __device__ inline bool take_fit(int32_t st, int32_t fit_cnt, int32_t n_new, int32_t best, int32_t head_count)
{
    const int32_t bar = best > head_count ? best : head_count;
    return (st == 0 || st == 2) && fit_cnt >= 4 && n_new >= bar;
}

// ---- the tail of an update, by every lane of the workgroup of entry ai (scene f of n_corr correspondences), which has counted n_new
// inliers of the refit, decided `take` (workgroup-uniform) and, where taken, written the mask(s): pose, head[f][0..1], best[f] and
// lo_taken[f] change together; taken or not, done[ai] |= scene_done at the scene's best: a flag that is set stays set.
__device__ inline void commit_fit(bool take, int st, int n_new, int best_prev, int n_corr, const double *fit_R, const double *fit_t, int64_t ai,
                                  double *io_R, double *io_t, int64_t f, int32_t *head, int32_t *best, int32_t *lo_taken, const int32_t *hyp_used,
                                  int32_t cap, double confidence, int32_t *done)
{
    if (take) {
        cvxn::take_pose(fit_R, fit_t, ai, io_R, io_t, f);
        if (threadIdx.x == 0) {
            head[f * 4] = st; head[f * 4 + 1] = n_new;
            best[f] = n_new;
            lo_taken[f] += 1;
        }
    }
    if (threadIdx.x == 0 && cvxna::scene_done(hyp_used[f], cap, take ? n_new : best_prev, n_corr, confidence)) done[ai] = 1;
}

} // namespace cvxnlo
