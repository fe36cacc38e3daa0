// ransac_guided_kernel.h -- guided RANSAC: minimal sets drawn from the best-ranked correspondences first (include/cvxpnpl_amd_ransac_guided.h,
// DESIGN.md section 20).  A scene's correspondences carry a quality; rank_quality_kernel turns it into order [n_total] int32, per scene a
// permutation of 0 .. M_f - 1, best first.  Hypothesis h of a scene then draws draw_minimal_set(n(h), seed_f, h) -- n(h) = cvxng::pool_size,
// which depends on (h, M_f, pool_full) alone -- and takes order[beg_f + pick[j]] as its correspondences; from h = pool_full on the draw is
// the uniform one of cvxn::uniform_hypothesis, used directly.  The Philox counter stays the hypothesis index within the scene, so a
// scene's hypotheses are the same whether they come in one launch (sample_guided_kernel) or in rounds (sample_guided_active_kernel, the
// layout of cvxna::sample_active_kernel).
//
// Slices are clamped to [0, n_total) by cvxn::scene_slice.  An order entry outside [0, M_f) never becomes an address: the hypothesis is
// written as the NaN hypothesis of a short scene (cvxn::write_point_set).  Every loop is bounded by M_f or a constant; nothing waits for another workgroup; no
// atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_common.h"
#include "ransac_guided_core.h"

namespace cvxng {

using cvxn::SCENE_BLOCK;
constexpr int RANK_TILE = SCENE_BLOCK; // keys per LDS tile of the ranking kernel: one per lane (2 KB)

// ---- ranking: grid (ceil(M_max / 256), scenes of the slab).  Lane m counts the records of its scene that rank before it -- the scene's
// keys go through LDS a tile at a time and are broadcast to the lanes -- and stores order[beg + rank] = m.  The order is strict and
// total, so every slot of the slice is written exactly once.  O(M_f^2) per scene.  A scene longer than the grid's x extent is covered by
// the workgroup-uniform stride loop.
struct RankArgs {
    int64_t scene0, n_scenes, n_total;
    const int64_t *off;
    const double *quality;   // [n_total]
    int32_t *order;          // [n_total]
};
__global__ void __launch_bounds__(SCENE_BLOCK) rank_quality_kernel(RankArgs a)
{
    __shared__ double tile[RANK_TILE];
    const int64_t f = a.scene0 + blockIdx.y;
    if (f >= a.n_scenes) return; // (block-uniform)
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const double *q = a.quality + sl.beg;
    const int64_t stride = (int64_t)gridDim.x * SCENE_BLOCK;
    for (int64_t m0 = (int64_t)blockIdx.x * SCENE_BLOCK; m0 < sl.n; m0 += stride) { // (block-uniform bounds: the barriers below are safe)
        const int64_t m = m0 + threadIdx.x;
        const bool live = m < sl.n;
        const double key = live ? quality_key(q[m]) : 0.0;
        int rank = 0;
        for (int base = 0; base < sl.n; base += RANK_TILE) {
            const int n = sl.n - base < RANK_TILE ? sl.n - base : RANK_TILE;
            __syncthreads();
            if ((int)threadIdx.x < n) tile[threadIdx.x] = quality_key(q[base + threadIdx.x]);
            __syncthreads();
            for (int i = 0; i < n; ++i) rank += ranks_before(tile[i], base + i, key, (int32_t)m) ? 1 : 0;
        }
        if (live) a.order[sl.beg + rank] = (int32_t)m; // rank <= M_f - 1: m does not rank before itself
    }
}

// one hypothesis: the four correspondences of hypothesis h (index within the scene) of a scene of sl.n >= 4 records, written as problem g
__device__ inline void guided_hypothesis(const cvxn::Slice sl, uint64_t seed, int32_t h, int32_t pool_full, const int32_t *order, const double *scene2,
                                         const double *scene3, int64_t g, int32_t *idx, double *p2, double *p3)
{
    int pick[4];
    bool ok = sl.n >= MINIMAL;
    if (ok) {
        cvxn::draw_minimal_set(pool_size(h, sl.n, pool_full), seed, (uint32_t)h, pick); // 0 .. n(h) - 1 <= M_f - 1 by construction
        if (h < pool_full) { // ranks to scene indices; from pool_full on the draw IS the scene index
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pick[j] = order[sl.beg + pick[j]];
                ok = ok && pick[j] >= 0 && pick[j] < sl.n;
            }
        }
    }
    // (!ok: no draw is possible, or the ranking is no ranking: the solve reports a non-finite pose)
    cvxn::write_point_set(ok, pick, sl.beg, scene2, scene3, g, idx, p2, p3);
}

// ---- sampling, every scene: the fixed layout, cvxn::hypothesis_K, then guided_hypothesis.  Grid (ceil(H / 256), scenes of the slab).
struct SampleGuidedArgs {
    int64_t scene0, n_scenes, n_total;
    int32_t n_hyp, pool_full;
    const int64_t *off;
    const uint64_t *seed;    // [n_scenes]
    const int32_t *order;    // [n_total] (not read when pool_full = 0)
    const double *s2, *s3;   // packed scenes
    const double *K;         // [n_scenes][9] or null
    int32_t *idx;            // [n_scenes * n_hyp][4] (optional)
    double *p2, *p3;         // [n_scenes * n_hyp][4][2], [..][4][3]
    double *Kh;              // [n_scenes * n_hyp][9] (with K)
};
__global__ void __launch_bounds__(SCENE_BLOCK) sample_guided_kernel(SampleGuidedArgs a)
{
    const int64_t f = a.scene0 + blockIdx.y;
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    if (f >= a.n_scenes || h >= a.n_hyp) return;
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const int64_t g = f * a.n_hyp + h;
    cvxn::hypothesis_K(a.K, f, a.Kh, g);
    guided_hypothesis(sl, a.seed[f], h, a.pool_full, a.order, a.s2, a.s3, g, a.idx, a.p2, a.p3);
}

// ---- sampling, the active scenes of a round: the scene indirection of cvxna::sample_active_kernel, cvxn::hypothesis_K, then guided_hypothesis.  Entry a is scene f = active[a],
// hypothesis h of the round is hypothesis hyp0 + h of the scene and problem a * n_round + h.  Grid (ceil(n_round / 256), entries of the slab).
struct SampleGuidedActiveArgs {
    int64_t act0, n_active, n_scenes, n_total;
    int32_t hyp0, n_round, pool_full;
    const int32_t *active;
    const int64_t *off;
    const uint64_t *seed;
    const int32_t *order;
    const double *s2, *s3;
    const double *K;
    int32_t *idx;            // [n_active * n_round][4] (optional)
    double *p2, *p3;
    double *Kh;
};
__global__ void __launch_bounds__(SCENE_BLOCK) sample_guided_active_kernel(SampleGuidedActiveArgs a)
{
    const int64_t ai = a.act0 + blockIdx.y;
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    if (ai >= a.n_active || h >= a.n_round) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // skipped, not clamped
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const int64_t g = ai * a.n_round + h;
    cvxn::hypothesis_K(a.K, f, a.Kh, g);
    guided_hypothesis(sl, a.seed[f], a.hyp0 + h, a.pool_full, a.order, a.s2, a.s3, g, a.idx, a.p2, a.p3); // hyp0 + h < cap: no wrap
}

} // namespace cvxng
