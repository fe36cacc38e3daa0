// ransac_pnpl_kernel.h -- RANSAC over point AND line correspondences, many scenes of different sizes in one launch sequence
// (include/cvxpnpl_amd_ransac_pnpl.h).  The steps of ransac_kernel.h for scenes that are TWO packed arrays: scene f
// is the points off_p[f] .. off_p[f+1] of [n_pts][2] / [n_pts][3] and the lines off_l[f] .. off_l[f+1] of [n_lines][2][2] /
// [n_lines][2][3]; every scene draws the same number H of hypotheses and hypothesis (f, h) is problem f * H + h.  A minimal set is four
// correspondences of the UNION of a scene's points and lines: its shape (4+0 .. 0+4) differs from lane to lane, so the sampling kernel
// assembles the set's cost itself and the minimal solves enter the solver at the cost seam (cvxpnpl_solve_cost_batch), as the refits do.
//
// Every kernel clamps both slices of a scene (cvxn::scene_slice): offsets live on the device and cannot be checked by the host entry
// points, and a wrong one must not become an access outside the packed arrays or masks.  All loops are bounded by H, P_f, L_f or a
// constant; every index into a packed array or into the F * H hypotheses is int64.
//
// The scene set, the line inlier predicate, a hypothesis from its draw to its cost (minimal_hypothesis), the scoring of one scene
// (score_scene) and the masks of one pose (block_inliers) are ransac_pnpl_common.h: the kernels of ransac_pnpl_adaptive_kernel.h use
// the same ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_assemble_core.h"
#include "ransac_pnpl_common.h"

namespace cvxnl {

// ---- sampling and minimal assembly: one lane per (scene, hypothesis), grid (ceil(H / 256), scenes).  The draw is that of
// cvxn::sample_scenes_kernel over M_f = P_f + L_f (cvxn::draw_minimal_set: same key, same counter); index c < P_f is point c, otherwise
// line c - P_f.  The lane assembles its set in place (cvxnl::minimal_hypothesis).  Q45 and B27 feed cvxpnpl_solve_cost_batch.
struct SampleArgs {
    SceneSet s;
    int64_t scene0;
    int32_t n_hyp;
    const uint64_t *seed;  // [n_scenes]
    int32_t *idx;          // [n_scenes * n_hyp][4] (optional)
    double *Q45, *B27;     // [n_scenes * n_hyp][45], [..][27]
};
__global__ void __launch_bounds__(BLOCK) sample_assemble_kernel(SampleArgs a)
{
    const int64_t f = a.scene0 + blockIdx.y;
    const int64_t h64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= a.s.n_scenes || h64 >= a.n_hyp) return;
    const int32_t h = (int32_t)h64;
    const Scene sc = scene_of(a.s, f);
    minimal_hypothesis(sc, a.seed[f], h, sc.P + sc.L, nullptr, f * a.n_hyp + h, a.idx, a.Q45, a.B27); // the pool is the scene, unranked
}

// ---- scoring: grid (ceil(H / 256), scenes), one lane per hypothesis of the workgroup's scene.  The scene's points go through LDS a tile
// at a time and are broadcast to the lanes (cvxn::score_points); then its lines, a tile of end points plus the NORMALISED
// image line, computed once per tile by the lane that stages the line.  count [n_scenes * n_hyp] = point inliers + line inliers.
struct ScoreArgs {
    SceneSet s;
    int64_t scene0;
    int32_t n_hyp;
    const double *R, *t;     // [n_scenes * n_hyp][9], [..][3]
    const int32_t *status;   // optional
    uint32_t usable_mask;    // bit s set: status s is scored
    double thresh;
    int32_t *count;
};
__global__ void __launch_bounds__(BLOCK) score_kernel(ScoreArgs a)
{
    __shared__ double tile[TILE_DOUBLES];
    const int64_t f = a.scene0 + blockIdx.y;
    if (f >= a.s.n_scenes) return; // (block-uniform)
    const int64_t h = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = h < a.n_hyp;
    const int64_t g = f * a.n_hyp + (live ? h : 0);
    const Scene sc = scene_of(a.s, f);
    Camera cam;
    cvxn::camera_load(a.R + g * 9, a.t + g * 3, sc.K, cam);
    const bool usable = cvxn::hypothesis_usable(live, a.status, g, a.usable_mask);
    const int cnt = score_scene(tile, sc, cam, usable, a.thresh);
    if (live) a.count[g] = cnt;
}

// ---- selection: ONE workgroup per scene, cvxn::select_scenes_kernel with two masks.  Arg-max of the scene's H counts with the LOWEST
// index winning a tie (cvxn::block_argmax), the number of certified hypotheses on the way, then the winner's pose and -- scored again by the workgroup's
// lanes -- its masks.  head[f] = { status of the pose, inliers (points + lines), index of the winner within the scene, certified }.
struct SelectArgs {
    SceneSet s;
    int32_t n_hyp;
    const int32_t *count;    // [n_scenes * n_hyp]
    const double *R, *t;
    const int32_t *status;
    double thresh;
    double *out_R, *out_t;   // [n_scenes][9], [n_scenes][3]
    int32_t *head;           // [n_scenes][4]
    uint8_t *mask_p, *mask_l; // [n_pts], [n_lines]
};
__global__ void __launch_bounds__(BLOCK) select_kernel(SelectArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ long long best_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.s.n_scenes) return;
    const int64_t g0 = f * a.n_hyp;
    const cvxn::Winner w = cvxn::block_argmax<int64_t>(a.count, a.status, g0, a.n_hyp, best_w, cert_w);
    const int hb = w.h, cert = w.cert;
    const int64_t gb = g0 + hb;
    const Scene sc = scene_of(a.s, f);
    Camera cam;
    cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, sc.K, cam);
    const int n_inl = block_inliers(cam, sc, a.thresh, a.mask_p + sc.beg_p, a.mask_l + sc.beg_l, red);
    cvxn::take_pose(a.R, a.t, gb, a.out_R, a.out_t, f);
    if (threadIdx.x == 0) { a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = hb; a.head[f * 4 + 3] = cert; }
}

// ---- consensus assembly: ONE wavefront per scene, cvxn::assemble_consensus_kernel over masked points, then masked lines.  The lanes
// stride over the scene's correspondences, each with Gram sums of its own; the 60 sums meet in a fixed-order XOR butterfly, after which
// every lane holds the same total: the result depends on the inputs only.  The centre is cvxas::centre of the first three selected
// 3D RECORDS in the order "points, then lines" (a line contributes its two end points): the centre cvxpnpl_assemble_batch uses on the
// gathered set.  Fewer than three CORRESPONDENCES taken, a singular N^T N or a singular K: NaN for that scene only.
struct ConsensusArgs {
    SceneSet s;
    const uint8_t *mask_p, *mask_l;  // [n_pts], [n_lines]
    double *B27, *Q45;               // [n_scenes][27], [n_scenes][45]
    int32_t *count;                  // [n_scenes]
};
__global__ void __launch_bounds__(64) assemble_consensus_kernel(ConsensusArgs a)
{
    const int64_t f = blockIdx.x;
    if (f >= a.s.n_scenes) return;
    const int lane = threadIdx.x;
    const Scene sc = scene_of(a.s, f);
    const uint8_t *mp = a.mask_p + sc.beg_p, *ml = a.mask_l + sc.beg_l;
    double Kc[9], Ki[9], det;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = sc.K[i];
    cvx::inv3(Kc, Ki, det);
    // the first three selected records: up to three points, then -- while fewer than three records -- up to two lines
    int fp[3] = {0, 0, 0}, fl[3] = {0, 0, 0};
    const int nfp = cvxas::wave_first(sc.P, 3, fp, [&](int64_t m) { return mp[m] != 0; });
    const int nfl = cvxas::wave_first(sc.L, cvxas::centre_lines_wanted(nfp), fl, [&](int64_t m) { return ml[m] != 0; });
    double c[3];
    cvxas::centre(nfp, fp, nfl, fl, sc.p3, sc.l3, c);
    cvx::Gram g;
    cvx::gram_zero(g);
    int n = 0;
    for (int64_t m = lane; m < sc.P; m += 64) {
        if (!mp[m]) continue;
        const double *x = sc.p2 + 2 * m, *X = sc.p3 + 3 * m;
        cvx::gram_add_point(g, Ki, x[0], x[1], X[0] - c[0], X[1] - c[1], X[2] - c[2]);
        ++n;
    }
    for (int64_t m = lane; m < sc.L; m += 64) {
        if (!ml[m]) continue;
        const double *x = sc.l2 + 4 * m, *e = sc.l3 + 6 * m;
        const double ab[4] = {x[0], x[1], x[2], x[3]};
        const double es[6] = {e[0] - c[0], e[1] - c[1], e[2] - c[2], e[3] - c[0], e[4] - c[1], e[5] - c[2]};
        cvx::gram_add_line(g, Ki, ab, es);
        ++n;
    }
    cvxas::wave_butterfly(g, n);
    double B[27], Q9[45];
    const bool ok = cvxas::finish(g, n, det, c, B, Q9);
    if (lane == 0) cvxas::store_cost(ok, B, Q9, n, f, a.B27, a.Q45, a.count); // (every lane holds the same values)
}

// ---- refit update: ONE workgroup per scene, the rule of cvxn::refit_update_scenes_kernel.  The refitted pose of the scene's consensus
// set is scored against the scene and TAKEN -- pose, status, both masks and count together -- when it is usable (status 0 or 2, fitted
// to at least four correspondences) and keeps at least the consensus it was fitted to; otherwise everything of the scene stays.
struct RefitArgs {
    SceneSet s;
    const double *fit_R, *fit_t;   // [n_scenes][9], [n_scenes][3]
    const int32_t *fit_status;     // [n_scenes]
    const int32_t *fit_cnt;        // [n_scenes] size of the set each was fitted to
    double thresh;
    double *io_R, *io_t;
    int32_t *head;                 // [n_scenes][4]
    uint8_t *mask_p, *mask_l;      // [n_pts], [n_lines]
};
__global__ void __launch_bounds__(BLOCK) refit_update_kernel(RefitArgs a)
{
    __shared__ int red[SCENE_WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.s.n_scenes) return;
    const Scene sc = scene_of(a.s, f);
    Camera cam;
    cvxn::camera_load(a.fit_R + f * 9, a.fit_t + f * 3, sc.K, cam);
    const int st = a.fit_status[f];
    const int n_new = block_inliers(cam, sc, a.thresh, nullptr, nullptr, red);
    const bool take = (st == 0 || st == 2) && a.fit_cnt[f] >= 4 && n_new >= a.head[f * 4 + 1]; // (workgroup-uniform)
    __syncthreads();
    if (!take) return;
    (void)block_inliers(cam, sc, a.thresh, a.mask_p + sc.beg_p, a.mask_l + sc.beg_l, red); // pose and masks change together
    cvxn::take_pose(a.fit_R, a.fit_t, f, a.io_R, a.io_t, f);
    if (threadIdx.x == 0) { a.head[f * 4] = st; a.head[f * 4 + 1] = n_new; }
}

} // namespace cvxnl
