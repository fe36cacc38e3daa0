// ransac_guided_core.h -- the two rules of guided RANSAC (include/cvxpnpl_amd_ransac_guided.h), ONE statement of
// each for the device (the kernels of ransac_guided_kernel.h) and the host (cvxpnpl_ransac_guided_pool_host, _rank_host): the size of the
// pool that hypothesis h draws from, and the order in which a scene's correspondences are ranked.  Nothing here knows what a
// correspondence is.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace cvxng {

constexpr int MINIMAL = 4; // correspondences of a minimal set

// T(n) = pool_full * C(n, 4) / C(M, 4): the number of the first pool_full uniform draws that fall inside the n best correspondences
// (the growth function of PROSAC).  float64, multiplications and divisions only, in exactly this order: nothing a compiler may contract
// to an FMA, so device, host and numpy take the same decisions.  Non-decreasing in n: every factor is, and rounding is monotone.
__host__ __device__ inline double pool_growth(int32_t n, int32_t M, int32_t pool_full)
{
    const double nd = (double)n, Md = (double)M;
    return (double)pool_full * ((nd / Md) * ((nd - 1.0) / (Md - 1.0)) * ((nd - 2.0) / (Md - 2.0)) * ((nd - 3.0) / (Md - 3.0)));
}

// n(h): the pool of hypothesis h >= 0 of a scene of M >= 4 ranked correspondences.  From pool_full on it is the whole scene;  before,
// min(n_T(h), 4 + h, M), n_T(h) the smallest n of 4 .. M with T(n) >= h + 1 (M when there is none), found by bisection: at most 31 steps.
__host__ __device__ inline int32_t pool_size(int32_t h, int32_t M, int32_t pool_full)
{
    if (h >= pool_full) return M;
    const double target = (double)h + 1.0;
    int32_t lo = MINIMAL, hi = M; // invariant: the answer lies in lo .. hi
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (pool_growth(mid, M, pool_full) >= target) hi = mid;
        else lo = mid + 1;
    }
    const int32_t grown = h < M - MINIMAL ? MINIMAL + h : M; // min(4 + h, M) without forming 4 + h
    return lo < grown ? lo : grown;
}

// the ranking: j comes before m when its key is greater, or equal with j < m.  The key is the quality, a NaN taken as -inf.  A strict
// total order, so the number of records before m is its rank and the ranks of a scene are a permutation; +0 and -0 tie.
__host__ __device__ inline double quality_key(double q) { return q != q ? -INFINITY : q; }
__host__ __device__ inline bool ranks_before(double key_j, int32_t j, double key_m, int32_t m)
{
    return key_j > key_m || (key_j == key_m && j < m);
}

} // namespace cvxng
