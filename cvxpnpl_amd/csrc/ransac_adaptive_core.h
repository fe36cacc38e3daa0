// ransac_adaptive_core.h -- the stopping rule of adaptive RANSAC (include/cvxpnpl_amd_ransac_adaptive.h), ONE
// statement of it for the device (round_update_kernel) and the host (cvxpnpl_ransac_adaptive_needed_host).  Nothing here knows what a
// correspondence is: I inliers of M, minimal sets of four drawn WITHOUT replacement (the partial Fisher-Yates of draw_minimal_set).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace cvxna {

constexpr int MINIMAL = 4; // correspondences of a minimal set

// N(I, M, confidence): the number of minimal sets after which one of them is all inliers with probability `confidence`, when I of the
// M correspondences are inliers:  q = prod_{j < 4} (I - j) / (M - j),  N = log(1 - confidence) / log1p(-q).  I < 4: no set can be all
// inliers, N = inf;  I >= M: the first set is, N = 0.  float64 throughout; the caller compares `drawn >= N` as floating point.
__host__ __device__ inline double hyp_needed(int32_t I, int32_t M, double confidence)
{
    if (I < MINIMAL || M < MINIMAL) return INFINITY;
    if (I >= M) return 0.0;
    double q = 1.0;
#pragma unroll
    for (int j = 0; j < MINIMAL; ++j) q *= (double)(I - j) / (double)(M - j);
    return log(1.0 - confidence) / log1p(-q);
}

// a scene is finished after `drawn` hypotheses, `best` the highest inlier count among them
__host__ __device__ inline bool scene_done(int32_t drawn, int32_t cap, int32_t best, int32_t M, double confidence)
{
    return drawn >= cap || (double)drawn >= hyp_needed(best, M, confidence);
}

__host__ __device__ inline bool bad_confidence(double c) { return !(c > 0.0 && c < 1.0); } // (NaN compares false)

} // namespace cvxna
