// ransac_pnpl_adaptive_kernel.h -- adaptive and guided RANSAC over point AND line correspondences
// (include/cvxpnpl_amd_ransac_pnpl_adaptive.h).  The rounds of ransac_adaptive_kernel.h and the ranked draws of
// ransac_guided_kernel.h for the scenes of ransac_pnpl_kernel.h: a round draws n_round further hypotheses for the scenes listed in
// active[0 .. n_active); entry a is scene f = active[a], hypothesis h of the round is hypothesis hyp0 + h of the scene -- the Philox
// counter of its draw -- and problem a * n_round + h of the round's minimal solve at the cost seam (the COMPACT layout).  What lasts
// over the rounds is indexed by the scene: pose [F], head [F][4], best [F], hyp_used [F] and the two packed masks.  A correspondence is
// an index into the UNION of a scene's points and lines (c < P_f: point c; otherwise line c - P_f; M_f = P_f + L_f), and the stopping
// rule (cvxna::scene_done) and the pool rule (cvxng::pool_size) run on that union.
//
// active[a] outside [0, n_scenes) makes the workgroup (or lane) return without a store: it is skipped, not clamped, because a clamped
// index would overwrite another scene.  Both slices of a scene are clamped (cvxnl::scene_of).  An order entry outside [0, M_f) never
// becomes an address.  Every loop is bounded by n_round, P_f, L_f, n_active or a constant; nothing waits for another workgroup; no
// atomics; every index into a packed array or into the n_active * n_round hypotheses is int64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_adaptive_core.h"
#include "ransac_guided_core.h"
#include "ransac_pnpl_common.h"

namespace cvxnla {

using cvxn::Camera;
using cvxnl::BLOCK;
using cvxnl::Scene;
using cvxnl::SceneSet;
using cvxn::SCENE_WAVES;

// ---- sampling and minimal assembly of a round: cvxnl::sample_assemble_kernel with the scene indirection, the pool and the ranking.
// Grid (ceil(n_round / 256), entries of the slab).  Hypothesis hs = hyp0 + h draws draw_minimal_set(pool_size(hs, M_f, pool_full),
// seed_f, hs); while hs < pool_full its set is order[beg_f + pick[j]], beg_f = beg_p + beg_l the scene's place in the union packing;
// from pool_full on the draw IS the union index and order is not read.  The rest is cvxnl::minimal_hypothesis: the identity active
// list with hyp0 = 0 and n_round = n_hyp gives the fixed layout f * n_hyp + h, and pool_full = 0 the bits of cvxnl::sample_assemble_kernel.
struct SampleArgs {
    SceneSet s;
    int64_t act0, n_active;
    int32_t hyp0, n_round, pool_full;
    const int32_t *active;
    const uint64_t *seed;  // [n_scenes]
    const int32_t *order;  // [n_pts + n_lines], union indices within the scene (not read when pool_full = 0)
    int32_t *idx;          // [n_active * n_round][4] (optional)
    double *Q45, *B27;     // [n_active * n_round][45], [..][27]
};
__global__ void __launch_bounds__(BLOCK) sample_assemble_active_kernel(SampleArgs a)
{
    const int64_t ai = a.act0 + blockIdx.y;
    const int64_t h64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (ai >= a.n_active || h64 >= a.n_round) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.s.n_scenes) return; // skipped, not clamped
    const int32_t hs = a.hyp0 + (int32_t)h64; // < cap: no wrap
    const Scene sc = cvxnl::scene_of(a.s, f);
    const int32_t M = sc.P + sc.L;
    // the pool and, before pool_full, the ranking: beg + rank < (beg_p + P) + (beg_l + L) <= n_pts + n_lines
    const int32_t pool = M >= cvxng::MINIMAL ? cvxng::pool_size(hs, M, a.pool_full) : M;
    const int32_t *ranked = hs < a.pool_full ? a.order + (sc.beg_p + sc.beg_l) : nullptr;
    cvxnl::minimal_hypothesis(sc, a.seed[f], hs, pool, ranked, ai * a.n_round + h64, a.idx, a.Q45, a.B27);
}

// ---- scoring of a round: the scene indirection and the compact layout, then cvxn::hypothesis_usable and cvxnl::score_scene.
// count [n_active * n_round].
struct ScoreArgs {
    SceneSet s;
    int64_t act0, n_active;
    int32_t n_round;
    const int32_t *active;
    const double *R, *t;     // [n_active * n_round][9], [..][3]
    const int32_t *status;   // optional
    uint32_t usable_mask;    // bit s set: status s is scored
    double thresh;
    int32_t *count;
};
__global__ void __launch_bounds__(BLOCK) score_pnpl_active_kernel(ScoreArgs a)
{
    __shared__ double tile[cvxnl::TILE_DOUBLES];
    const int64_t ai = a.act0 + blockIdx.y;
    if (ai >= a.n_active) return; // (block-uniform)
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.s.n_scenes) return; // (block-uniform) skipped, not clamped
    const int64_t h = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = h < a.n_round;
    const int64_t g = ai * a.n_round + (live ? h : 0);
    const Scene sc = cvxnl::scene_of(a.s, f);
    Camera cam;
    cvxn::camera_load(a.R + g * 9, a.t + g * 3, sc.K, cam);
    const bool usable = cvxn::hypothesis_usable(live, a.status, g, a.usable_mask);
    const int cnt = cvxnl::score_scene(tile, sc, cam, usable, a.thresh);
    if (live) a.count[g] = cnt;
}

// ---- the round's update: ONE workgroup per active scene, cvxna::round_update_kernel with two masks.  The arg-max of the round's counts
// (cvxn::block_argmax: lowest index on a tie), merged into the scene's running best by a STRICTLY greater count, so that an earlier
// hypothesis keeps a tie over the rounds as it does within one.  best[f] is the count the scoring kernel gave the running winner
// (head[f][1] is the size of the masks it was scored again for).  On replacement pose, head[f][0..2] and the scene's slices of both masks
// change together; certified hypotheses accumulate in head[f][3]; then the stopping rule on M_f = P_f + L_f.
struct UpdateArgs {
    SceneSet s;
    int64_t n_active;
    int32_t hyp0, n_round, cap;
    double confidence;
    const int32_t *active;
    const int32_t *count;     // [n_active * n_round]
    const double *R, *t;
    const int32_t *status;
    double thresh;
    double *out_R, *out_t;    // [n_scenes][9], [n_scenes][3]
    int32_t *head;            // [n_scenes][4]
    int32_t *best;            // [n_scenes]
    uint8_t *mask_p, *mask_l; // [n_pts], [n_lines]
    int32_t *hyp_used;        // [n_scenes]
    int32_t *done;            // [n_active]
};
__global__ void __launch_bounds__(BLOCK) update_pnpl_active_kernel(UpdateArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ long long best_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.s.n_scenes) return; // (block-uniform) skipped, not clamped
    const int64_t g0 = ai * a.n_round;
    const cvxn::Winner w = cvxn::block_argmax<int>(a.count, a.status, g0, a.n_round, best_w, cert_w);
    const int hb = w.h, cert = w.cert;
    const int cnt_round = w.count;
    const int cnt_prev = a.best[f];
    const bool replace = cnt_round > cnt_prev; // (workgroup-uniform)
    const Scene sc = cvxnl::scene_of(a.s, f);
    if (replace) {
        const int64_t gb = g0 + hb;
        Camera cam;
        cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, sc.K, cam);
        const int n_inl = cvxnl::block_inliers(cam, sc, a.thresh, a.mask_p + sc.beg_p, a.mask_l + sc.beg_l, red);
        cvxn::take_pose(a.R, a.t, gb, a.out_R, a.out_t, f);
        if (threadIdx.x == 0) { a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = a.hyp0 + hb; a.best[f] = cnt_round; }
    }
    if (threadIdx.x == 0) {
        const int drawn = a.hyp0 + a.n_round;
        a.head[f * 4 + 3] += cert;
        a.hyp_used[f] = drawn;
        a.done[ai] = cvxna::scene_done(drawn, a.cap, replace ? cnt_round : cnt_prev, sc.P + sc.L, a.confidence) ? 1 : 0;
    }
}

} // namespace cvxnla
