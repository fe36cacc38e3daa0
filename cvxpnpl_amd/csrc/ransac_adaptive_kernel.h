// ransac_adaptive_kernel.h -- RANSAC over many scenes with a hypothesis budget PER SCENE, solved in rounds
// (include/cvxpnpl_amd_ransac_adaptive.h).  ransac_kernel.h gives every scene the same H hypotheses; here a round
// draws n_round further hypotheses for the scenes that are still ACTIVE, listed in active[0 .. n_active): entry a is scene f = active[a],
// and hypothesis h of the round is problem a * n_round + h of the round's minimal solve -- the COMPACT layout, which holds nothing of a
// finished scene.  The hypothesis' index within its scene is hyp0 + h; it is the Philox counter of the draw, so a scene's hypotheses
// are the same whether they are drawn in one launch or in rounds.  What lasts over the rounds is full-size, indexed by the scene:
// pose [F], head [F][4], best [F], hyp_used [F] and the packed mask.
//
// active[a] outside [0, n_scenes) makes the workgroup (or lane) return without a store: it is skipped, not clamped, because a clamped
// index would overwrite another scene.  Slices are clamped to [0, n_total) as in ransac_kernel.h.  Every loop is bounded by n_round,
// M_f, n_active or a constant; nothing waits for another workgroup; no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_adaptive_core.h"
#include "ransac_common.h"

namespace cvxna {

using cvxn::SCENE_BLOCK;
using cvxn::SCENE_WAVES;
using cvxn::POINT_TILE;

// ---- start of a call: every scene active, nothing drawn.  One lane per scene.
struct InitArgs {
    int64_t n_scenes;
    int32_t *active;     // [n_scenes]
    int32_t *n_active;   // [1]
    int32_t *head;       // [n_scenes][4]
    int32_t *best;       // [n_scenes]
    int32_t *hyp_used;   // [n_scenes]
};
__global__ void __launch_bounds__(SCENE_BLOCK) adaptive_init_kernel(InitArgs a)
{
    const int64_t f = (int64_t)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (f == 0) a.n_active[0] = (int32_t)a.n_scenes;
    if (f >= a.n_scenes) return;
    a.active[f] = (int32_t)f;
    a.head[f * 4] = 3; a.head[f * 4 + 1] = -1; a.head[f * 4 + 2] = 0; a.head[f * 4 + 3] = 0;
    a.best[f] = -1; // below every count: the first round always replaces
    a.hyp_used[f] = 0;
}

// ---- sampling: the scene indirection, then cvxn::hypothesis_K and cvxn::uniform_hypothesis with the counter hyp0 + h.
// Grid (ceil(n_round / 256), active scenes of the slab).
struct SampleActiveArgs {
    int64_t act0, n_active, n_scenes, n_total;
    int32_t hyp0, n_round;
    const int32_t *active;
    const int64_t *off;
    const uint64_t *seed;    // [n_scenes]
    const double *s2, *s3;   // packed scenes
    const double *K;         // [n_scenes][9] or null
    int32_t *idx;            // [n_active * n_round][4] (optional)
    double *p2, *p3;         // [n_active * n_round][4][2], [..][4][3]
    double *Kh;              // [n_active * n_round][9] (with K)
};
__global__ void __launch_bounds__(SCENE_BLOCK) sample_active_kernel(SampleActiveArgs a)
{
    const int64_t ai = a.act0 + blockIdx.y;
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    if (ai >= a.n_active || h >= a.n_round) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return;
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const int64_t g = ai * a.n_round + h;
    cvxn::hypothesis_K(a.K, f, a.Kh, g);
    cvxn::uniform_hypothesis(sl, a.seed[f], a.hyp0 + h, a.s2, a.s3, g, a.idx, a.p2, a.p3);
}

// ---- scoring: the scene indirection, then cvxn::hypothesis_usable and cvxn::score_points (the scene through LDS a tile at a time).
// count [n_active * n_round].
struct ScoreActiveArgs {
    int64_t act0, n_active, n_scenes, n_total;
    int32_t n_round;
    const int32_t *active;
    const int64_t *off;
    const double *R, *t;     // [n_active * n_round][9], [..][3]
    const int32_t *status;   // optional
    uint32_t usable_mask;    // bit s set: status s is scored
    const double *K;         // [9] or [n_scenes][9]
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    int32_t *count;
};
__global__ void __launch_bounds__(SCENE_BLOCK) score_active_kernel(ScoreActiveArgs a)
{
    __shared__ double scene[POINT_TILE * 5];
    const int64_t ai = a.act0 + blockIdx.y;
    if (ai >= a.n_active) return; // (block-uniform)
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform)
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    const bool live = h < a.n_round;
    const int64_t g = ai * a.n_round + (live ? h : 0);
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    cvxn::Camera cam;
    cvxn::camera_load(a.R + g * 9, a.t + g * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const bool usable = cvxn::hypothesis_usable(live, a.status, g, a.usable_mask);
    const double th2 = a.thresh * a.thresh;
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    const int cnt = cvxn::score_points<int>(scene, sl.n, s2, s3, cam, usable, th2);
    if (live) a.count[g] = cnt;
}

// ---- the round's update: ONE workgroup per active scene.  The arg-max of the round's counts (cvxn::block_argmax: lowest index on a
// tie), merged into the scene's running best by a STRICTLY greater count, so that an earlier hypothesis keeps a
// tie over the rounds as it does within one.  best[f] is the count the scoring kernel gave the running winner (head[f][1] is the size of
// the mask it was scored again for: the same for a usable winner, and not 0 for an unusable one).  On replacement pose, head[f][0..2]
// and the scene's slice of the mask change together; certified hypotheses accumulate in head[f][3]; then the stopping rule.
struct RoundUpdateArgs {
    int64_t n_active, n_scenes, n_total;
    int32_t hyp0, n_round, cap;
    double confidence;
    const int32_t *active;
    const int64_t *off;
    const int32_t *count;    // [n_active * n_round]
    const double *R, *t;
    const int32_t *status;
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *out_R, *out_t;   // [n_scenes][9], [n_scenes][3]
    int32_t *head;           // [n_scenes][4]
    int32_t *best;           // [n_scenes]
    uint8_t *mask;           // [n_total]
    int32_t *hyp_used;       // [n_scenes]
    int32_t *done;           // [n_active]
};
__global__ void __launch_bounds__(SCENE_BLOCK) round_update_kernel(RoundUpdateArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ long long best_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform) skipped, not clamped
    const int64_t g0 = ai * a.n_round;
    const cvxn::Winner w = cvxn::block_argmax<int>(a.count, a.status, g0, a.n_round, best_w, cert_w);
    const int hb = w.h, cert = w.cert;
    const int cnt_round = w.count;
    const int cnt_prev = a.best[f];
    const bool replace = cnt_round > cnt_prev; // (workgroup-uniform)
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    if (replace) {
        const int64_t gb = g0 + hb;
        cvxn::Camera cam;
        cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
        const int n_inl = cvxn::block_inliers(cam, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, a.thresh * a.thresh, a.mask + sl.beg, red);
        cvxn::take_pose(a.R, a.t, gb, a.out_R, a.out_t, f);
        if (threadIdx.x == 0) { a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = a.hyp0 + hb; a.best[f] = cnt_round; }
    }
    if (threadIdx.x == 0) {
        const int drawn = a.hyp0 + a.n_round;
        a.head[f * 4 + 3] += cert;
        a.hyp_used[f] = drawn;
        a.done[ai] = scene_done(drawn, a.cap, replace ? cnt_round : cnt_prev, sl.n, a.confidence) ? 1 : 0;
    }
}

// ---- compaction: ONE workgroup.  active_next = the entries of active whose scene is not done, in order (stable), and their number.
// Ballots and prefix sums over chunks of 256 with a running base: the result depends on nothing but the inputs.  An entry outside
// [0, n_scenes) was skipped by the round (its done flag was never written) and is dropped here.
struct CompactArgs {
    int64_t n_active, n_scenes;
    const int32_t *active;
    const int32_t *done;     // [n_active]
    int32_t *active_next;    // [n_active]
    int32_t *n_active_next;  // [1]
};
__global__ void __launch_bounds__(SCENE_BLOCK) compact_active_kernel(CompactArgs a)
{
    __shared__ int wave_n[SCENE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < a.n_active; c0 += SCENE_BLOCK) { // ceil(n_active / 256) passes
        const int64_t i = c0 + threadIdx.x;
        int32_t f = -1;
        bool keep = false;
        if (i < a.n_active) {
            f = a.active[i];
            keep = f >= 0 && f < a.n_scenes && a.done[i] == 0;
        }
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1ull)); // kept lanes of this wave in front of this one
        __syncthreads(); // (the previous pass has read wave_n)
        if (lane == 0) wave_n[wave] = __popcll(b);
        __syncthreads();
        int front = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < SCENE_WAVES; ++wv) {
            front += wv < wave ? wave_n[wv] : 0;
            total += wave_n[wv];
        }
        if (keep) a.active_next[base + front + before] = f; // base + front + before <= i: inside [0, n_active)
        base += total;
    }
    if (threadIdx.x == 0) a.n_active_next[0] = (int32_t)base;
}

} // namespace cvxna
