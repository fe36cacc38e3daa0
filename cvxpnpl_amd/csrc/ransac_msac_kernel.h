// ransac_msac_kernel.h -- MSAC scoring for RANSAC over many scenes (include/cvxpnpl_amd_ransac_msac.h): the
// hypothesis of a scene is selected by its GAIN, sum over the inliers of (thresh^2 - r^2) / thresh^2, instead of by its inlier count.
// The scoring, selection and round-update kernels of ransac_kernel.h and ransac_adaptive_kernel.h, restated for (gain, count): the scene
// conventions are theirs -- scene f is the clamped slice off[f] .. off[f+1] of the packed correspondences (cvxn::scene_slice), hypothesis
// (f, h) is problem f * n_hyp + h of a fixed budget, (a, h) is problem a * n_round + h of a round (the COMPACT layout), an entry of the
// active list outside [0, n_scenes) is skipped, not clamped.  The arithmetic is ransac_msac_core.h; the mask of a winner, its size and
// the pose taken are cvxn::block_inliers and cvxn::take_pose as they stand.  Every loop is bounded by n_hyp, n_round, M_f or a constant;
// nothing waits for another workgroup; no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_adaptive_core.h"
#include "ransac_common.h"
#include "ransac_msac_core.h"

namespace cvxnm {

using cvxn::SCENE_BLOCK;
using cvxn::SCENE_WAVES;
using cvxn::POINT_TILE;

// ---- scoring, one pose per LANE: the scene's n points go through LDS a tile at a time and are broadcast to the lanes (a ds_read of a
// wave-uniform address), as in cvxn::score_points.  A lane adds its terms SERIALLY in scene order: the sum does not depend on the tile
// size, the grid or the kernel.  Every lane of the workgroup calls it (barriers).
__device__ inline Sum score_points_msac(double *tile /* LDS, POINT_TILE * 5 */, int n_pts, const double *s2, const double *s3, const Cam &cam, bool usable,
                                        double th2)
{
    Sum acc{0.0, 0};
    for (int base = 0; base < n_pts; base += POINT_TILE) {
        const int n = n_pts - base < POINT_TILE ? n_pts - base : POINT_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += SCENE_BLOCK) {
            const int64_t m = (int64_t)base + i;
            tile[i * 5 + 0] = s3[m * 3 + 0];
            tile[i * 5 + 1] = s3[m * 3 + 1];
            tile[i * 5 + 2] = s3[m * 3 + 2];
            tile[i * 5 + 3] = s2[m * 2 + 0];
            tile[i * 5 + 4] = s2[m * 2 + 1];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            sum_add(acc, usable, point_gain(cam, tile[i * 5], tile[i * 5 + 1], tile[i * 5 + 2], tile[i * 5 + 3], tile[i * 5 + 4], th2));
    }
    return acc;
}

// ---- scoring of a fixed budget: grid (ceil(n_hyp / 256), scenes), one lane per hypothesis of the workgroup's scene.
// gain, count [n_scenes * n_hyp]; an unusable hypothesis gains 0.0 and counts 0.
struct ScoreScenesMsacArgs {
    int64_t scene0, n_scenes, n_total;
    int32_t n_hyp;
    const int64_t *off;
    const double *R, *t;     // [n_scenes * n_hyp][9], [..][3]
    const int32_t *status;   // optional
    uint32_t usable_mask;    // bit s set: status s is scored
    const double *K;         // [9] or [n_scenes][9]
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *gain;
    int32_t *count;
};
__global__ void __launch_bounds__(SCENE_BLOCK) score_scenes_msac_kernel(ScoreScenesMsacArgs a)
{
    __shared__ double scene[POINT_TILE * 5];
    const int64_t f = a.scene0 + blockIdx.y;
    if (f >= a.n_scenes) return; // (block-uniform)
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    const bool live = h < a.n_hyp;
    const int64_t g = f * a.n_hyp + (live ? h : 0);
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    Cam cam;
    cam_load(a.R + g * 9, a.t + g * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const bool usable = hypothesis_usable(live, a.status, g, a.usable_mask);
    const double th2 = a.thresh * a.thresh;
    const Sum acc = score_points_msac(scene, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, cam, usable, th2);
    if (live) { a.gain[g] = sum_gain(acc, th2); a.count[g] = acc.n; }
}

// ---- scoring of a round: the scene indirection of cvxna::score_active_kernel, then the same.  gain, count [n_active * n_round].
struct ScoreActiveMsacArgs {
    int64_t act0, n_active, n_scenes, n_total;
    int32_t n_round;
    const int32_t *active;
    const int64_t *off;
    const double *R, *t;     // [n_active * n_round][9], [..][3]
    const int32_t *status;   // optional
    uint32_t usable_mask;
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *gain;
    int32_t *count;
};
__global__ void __launch_bounds__(SCENE_BLOCK) score_active_msac_kernel(ScoreActiveMsacArgs a)
{
    __shared__ double scene[POINT_TILE * 5];
    const int64_t ai = a.act0 + blockIdx.y;
    if (ai >= a.n_active) return; // (block-uniform)
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform) skipped, not clamped
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    const bool live = h < a.n_round;
    const int64_t g = ai * a.n_round + (live ? h : 0);
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    Cam cam;
    cam_load(a.R + g * 9, a.t + g * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const bool usable = hypothesis_usable(live, a.status, g, a.usable_mask);
    const double th2 = a.thresh * a.thresh;
    const Sum acc = score_points_msac(scene, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, cam, usable, th2);
    if (live) { a.gain[g] = sum_gain(acc, th2); a.count[g] = acc.n; }
}

// ---- the arg-max of the n gains gain[g0 .. g0 + n) by one workgroup under `better` (the LOWEST index on an exact tie), and the number
// of certified hypotheses (status 0) on the way.  A lane keeps the best (gain, index) of its stride; the wave's best comes down a
// shuffle tree -- the double moves as its two halves, the index beside it --, the SCENE_WAVES partials meet in LDS and every lane
// combines them in the same order, so every lane gets the same winner.  h is inside [0, n) whatever the gains hold; gain is the
// winner's as the ordering read it (gain_read).
struct GainWinner { int h; double gain; int cert; };
__device__ inline GainWinner block_argmax_gain(const double *gain, const int32_t *status, int64_t g0, int n, double *gain_w, int *h_w, int *cert_w /* LDS, SCENE_WAVES each */)
{
    double bg = 0.0;
    int bh = 0x7fffffff, cert = 0; // (no hypothesis: loses against every index)
    for (int h = threadIdx.x; h < n; h += SCENE_BLOCK) {
        const double g = gain_read(gain[g0 + h]);
        if (better(g, h, bg, bh)) { bg = g; bh = h; }
        cert += status[g0 + h] == 0 ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double og = __shfl_down(bg, o);
        const int oh = __shfl_down(bh, o);
        if (better(og, oh, bg, bh)) { bg = og; bh = oh; }
        cert += __shfl_down(cert, o);
    }
    if ((threadIdx.x & 63) == 0) { gain_w[threadIdx.x >> 6] = bg; h_w[threadIdx.x >> 6] = bh; cert_w[threadIdx.x >> 6] = cert; }
    __syncthreads();
    bg = gain_w[0]; bh = h_w[0]; cert = cert_w[0];
#pragma unroll
    for (int wv = 1; wv < SCENE_WAVES; ++wv) {
        if (better(gain_w[wv], h_w[wv], bg, bh)) { bg = gain_w[wv]; bh = h_w[wv]; }
        cert += cert_w[wv];
    }
    bh = bh < 0 || bh >= n ? 0 : bh;
    return GainWinner{bh, bg, cert};
}

// ---- selection: ONE workgroup per scene, what cvxn::select_scenes_kernel does with the gains deciding.  head[f] = { status of the
// pose, inliers (the size of the mask), index of the winner within the scene, certified hypotheses }; score[f] = the winner's gain.
struct SelectScenesMsacArgs {
    int64_t n_scenes, n_total;
    int32_t n_hyp;
    const int64_t *off;
    const double *gain;      // [n_scenes * n_hyp]
    const double *R, *t;
    const int32_t *status;
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *out_R, *out_t;   // [n_scenes][9], [n_scenes][3]
    int32_t *head;           // [n_scenes][4]
    uint8_t *mask;           // [n_total]
    double *score;           // [n_scenes]
};
__global__ void __launch_bounds__(SCENE_BLOCK) select_scenes_msac_kernel(SelectScenesMsacArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ double gain_w[SCENE_WAVES];
    __shared__ int h_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    const int64_t g0 = f * a.n_hyp;
    const GainWinner w = block_argmax_gain(a.gain, a.status, g0, a.n_hyp, gain_w, h_w, cert_w);
    const int64_t gb = g0 + w.h;
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    cvxn::Camera cam;
    cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const int n_inl = cvxn::block_inliers(cam, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, a.thresh * a.thresh, a.mask + sl.beg, red);
    cvxn::take_pose(a.R, a.t, gb, a.out_R, a.out_t, f);
    if (threadIdx.x == 0) {
        a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = w.h; a.head[f * 4 + 3] = w.cert;
        a.score[f] = w.gain;
    }
}

// ---- start of an adaptive call: best_gain[f] = -1, below every gain, so that the first round always replaces.  (The rest of the state
// is cvxna::adaptive_init_kernel's, which does not know best_gain.)  One lane per scene.
struct InitMsacArgs {
    int64_t n_scenes;
    double *best_gain;       // [n_scenes]
};
__global__ void __launch_bounds__(SCENE_BLOCK) msac_init_kernel(InitMsacArgs a)
{
    const int64_t f = (int64_t)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (f < a.n_scenes) a.best_gain[f] = -1.0;
}

// ---- the round's update: ONE workgroup per active scene, the rule of cvxna::round_update_kernel with the gains deciding.  The round's
// winner replaces the scene's running one only by a STRICTLY greater gain, so that an earlier hypothesis keeps a tie over the rounds as
// it does within one; then pose, head[f][0..2], the scene's slice of the mask, best[f] -- the COUNT the scoring kernel gave that
// winner -- and best_gain[f] change together.  Certified hypotheses accumulate in head[f][3].  The stopping rule is unchanged: it reads
// the inlier count of the running winner.
struct RoundUpdateMsacArgs {
    int64_t n_active, n_scenes, n_total;
    int32_t hyp0, n_round, cap;
    double confidence;
    const int32_t *active;
    const int64_t *off;
    const double *gain;      // [n_active * n_round]
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
    double *best_gain;       // [n_scenes]
    uint8_t *mask;           // [n_total]
    int32_t *hyp_used;       // [n_scenes]
    int32_t *done;           // [n_active]
};
__global__ void __launch_bounds__(SCENE_BLOCK) round_update_msac_kernel(RoundUpdateMsacArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ double gain_w[SCENE_WAVES];
    __shared__ int h_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform) skipped, not clamped
    const int64_t g0 = ai * a.n_round;
    const GainWinner w = block_argmax_gain(a.gain, a.status, g0, a.n_round, gain_w, h_w, cert_w);
    const int64_t gb = g0 + w.h;
    const int cnt_round = a.count[gb];
    const int cnt_prev = a.best[f];
    const bool replace = w.gain > a.best_gain[f]; // (workgroup-uniform; every lane has read both before lane 0 stores)
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    if (replace) {
        cvxn::Camera cam;
        cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
        const int n_inl = cvxn::block_inliers(cam, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, a.thresh * a.thresh, a.mask + sl.beg, red);
        cvxn::take_pose(a.R, a.t, gb, a.out_R, a.out_t, f);
        if (threadIdx.x == 0) {
            a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = a.hyp0 + w.h;
            a.best[f] = cnt_round; a.best_gain[f] = w.gain;
        }
    }
    if (threadIdx.x == 0) {
        const int drawn = a.hyp0 + a.n_round;
        a.head[f * 4 + 3] += w.cert;
        a.hyp_used[f] = drawn;
        a.done[ai] = cvxna::scene_done(drawn, a.cap, replace ? cnt_round : cnt_prev, sl.n, a.confidence) ? 1 : 0;
    }
}

} // namespace cvxnm
