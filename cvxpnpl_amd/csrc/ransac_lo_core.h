// ransac_lo_core.h -- the rules of local optimisation in adaptive RANSAC (include/cvxpnpl_amd_ransac_lo.h), ONE
// statement of them for the device (lo_assemble_active_kernel, lo_update_active_kernel) and the host (cvxpnpl_ransac_lo_assemble_host):
// which correspondences a step takes, the centre of their Gram sums, which lane adds which correspondence and in which order the partial
// sums meet, and when a refitted pose is taken.
//
// The assembly of one active entry, by LANES = 256 lanes in four wavefronts:
//   taken(m)  = the inlier predicate of cvxn::is_inlier at the scene's running pose, threshold th2 = (thresh * m_k)^2
//   centre    = cvx::shift_centre of the first three taken correspondences in scene order (any centre is exact)
//   lane l    adds the taken correspondences m = l, l + 256, l + 512, ... in that order           (lane_sums)
//   a wave    adds its 64 lanes' sums in the XOR butterfly o = 1, 2, 4, 8, 16, 32                 (v <- v + v[lane ^ o])
//   the entry adds the four waves' sums in wave order, ((w0 + w1) + w2) + w3                      (waves_total)
// so the 60 sums depend on the inputs alone.  On the device the camera and the predicate ARE cvxn::camera_load and cvxn::is_inlier; those
// are device-only, so the host build restates them expression by expression (as ransac_msac_core.h does).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_adaptive_core.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxnlo {

constexpr int LANES = cvxn::SCENE_BLOCK;  // lanes of an assembly: the family's workgroup
constexpr int WAVES = cvxn::SCENE_WAVES;
constexpr int GRAM = 60;                  // doubles of a cvx::Gram
static_assert(sizeof(cvx::Gram) == GRAM * sizeof(double), "a Gram is 60 doubles and nothing else");

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

// ---- the centre: cvx::shift_centre of the nf <= 3 first taken correspondences first[0 .. nf) (scene order); none taken: the origin
__host__ __device__ inline void centre(int nf, const int *first, const double *s3, double *c)
{
    c[0] = c[1] = c[2] = 0.0;
    if (nf <= 0) return;
    double first3[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { // (entries beyond nf repeat the first record and are not read by shift_centre)
        const int m = k < nf ? first[k] : first[0];
        first3[3 * k] = s3[3 * m]; first3[3 * k + 1] = s3[3 * m + 1]; first3[3 * k + 2] = s3[3 * m + 2];
    }
    cvx::shift_centre(nf, first3, 0, nullptr, c);
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

// ---- sum e of the entry from the WAVES wave sums part[w * stride + e], in wave order
__host__ __device__ inline double waves_total(const double *part, int stride, int e)
{
    double tot = part[e];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) tot += part[w * stride + e];
    return tot;
}

// ---- B27 and Q45 of the entry from its total sums: cvx::gram_finish, the centre put back into B; NaN for fewer than three taken, a
// singular N^T N or a singular K -- what cvxn::assemble_consensus_kernel reports.  Returns whether the cost is usable.
__host__ __device__ inline bool finish(const cvx::Gram &g, int n, double det, const double *c, double *B, double *Q9)
{
    const bool ok = n >= 3 && cvx::gram_finish(g, B, Q9) && (det == det) && det != 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j];
    return ok;
}

// ---- the update: a refitted pose of status st, fitted to fit_cnt correspondences and counting n_new inliers at thresh, is TAKEN when it
// is usable and holds at least the running best -- the rule of cvxn::refit_update_scenes_kernel: the non-minimal fit wins a tie.
__host__ __device__ inline bool take_fit(int32_t st, int32_t fit_cnt, int32_t n_new, int32_t best, int32_t head_count)
{
    const int32_t bar = best > head_count ? best : head_count;
    return (st == 0 || st == 2) && fit_cnt >= 4 && n_new >= bar;
}

} // namespace cvxnlo
