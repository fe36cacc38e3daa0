// ransac_kernel.h -- RANSAC over MANY scenes of different sizes in one launch sequence (include/cvxpnpl_amd_ransac.h, DESIGN.md
// section 13).  score_kernel.h holds the same five steps for ONE scene; here scene f is the slice off[f] .. off[f+1] of the packed
// correspondences [n_total][2] / [n_total][3], every scene draws the same number H of hypotheses, and hypothesis (f, h) is problem
// f * H + h of the minimal solve.  Only the scenes are ragged, and a scene is only ever streamed.
//
// Every kernel clamps a scene's slice to [0, n_total): offsets live on the device and cannot be checked by the host entry points, and
// a wrong one must not become a store outside the packed mask.  All loops are bounded by H, M_f or a constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_assemble_core.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxn {

// (SCENE_BLOCK, the lanes of every workgroup here, SCENE_WAVES, POINT_TILE and the steps the kernels call: ransac_common.h; those of the
// consensus assembly: ransac_assemble_core.h)

// ---- sampling: one lane per (scene, hypothesis), grid (ceil(H / 256), scenes).  The draw of cvxs::sample_sets_kernel for k = 4 over the
// scene's own M_f, with the scene's own seed as the Philox key and the hypothesis index WITHIN the scene as the counter: scene f draws
// what cvxpnpl_sample_minimal_sets(scene f, H, 4, seed_f) draws.
struct SampleScenesArgs {
    int64_t scene0, n_scenes, n_total;
    int32_t n_hyp;
    const int64_t *off;
    const uint64_t *seed;    // [n_scenes]
    const double *s2, *s3;   // packed scenes
    const double *K;         // [n_scenes][9] or null
    int32_t *idx;            // [n_scenes * n_hyp][4] (optional)
    double *p2, *p3;         // [n_scenes * n_hyp][4][2], [..][4][3]
    double *Kh;              // [n_scenes * n_hyp][9] (with K)
};
__global__ void __launch_bounds__(SCENE_BLOCK) sample_scenes_kernel(SampleScenesArgs a)
{
    const int64_t f = a.scene0 + blockIdx.y;
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    if (f >= a.n_scenes || h >= a.n_hyp) return;
    const Slice sl = scene_slice(a.off, f, a.n_total);
    const int64_t g = f * a.n_hyp + h;
    hypothesis_K(a.K, f, a.Kh, g);
    uniform_hypothesis(sl, a.seed[f], h, a.s2, a.s3, g, a.idx, a.p2, a.p3);
}

// ---- scoring: grid (ceil(H / 256), scenes), one lane per hypothesis of the workgroup's scene; the scene is staged through LDS a tile at
// a time and broadcast to the lanes (score_points), a hypothesis outside usable_mask scoring nothing (hypothesis_usable).  count [n_scenes * n_hyp].
struct ScoreScenesArgs {
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
    int32_t *count;
};
__global__ void __launch_bounds__(SCENE_BLOCK) score_scenes_kernel(ScoreScenesArgs a)
{
    __shared__ double scene[POINT_TILE * 5];
    const int64_t f = a.scene0 + blockIdx.y;
    if (f >= a.n_scenes) return; // (block-uniform)
    const int32_t h = (int32_t)(blockIdx.x * SCENE_BLOCK + threadIdx.x);
    const bool live = h < a.n_hyp;
    const int64_t g = f * a.n_hyp + (live ? h : 0);
    const Slice sl = scene_slice(a.off, f, a.n_total);
    Camera cam;
    camera_load(a.R + g * 9, a.t + g * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const bool usable = hypothesis_usable(live, a.status, g, a.usable_mask);
    const double th2 = a.thresh * a.thresh;
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    const int cnt = score_points<int>(scene, sl.n, s2, s3, cam, usable, th2);
    if (live) a.count[g] = cnt;
}

// ---- selection: ONE workgroup per scene.  Arg-max of the scene's H counts with the LOWEST index winning a tie, the number of certified
// hypotheses on the way, then the winner's pose and -- scored again by the workgroup's lanes -- its mask in the scene's slice of the
// packed mask.  (The arg-max is a copy of cvxn::block_argmax: DESIGN.md section 13 says why.)  head[f] = { status of the pose, inliers, index of the winner within the scene, certified hypotheses }.
struct SelectScenesArgs {
    int64_t n_scenes, n_total;
    int32_t n_hyp;
    const int64_t *off;
    const int32_t *count;    // [n_scenes * n_hyp]
    const double *R, *t;
    const int32_t *status;
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *out_R, *out_t;   // [n_scenes][9], [n_scenes][3]
    int32_t *head;           // [n_scenes][4]
    uint8_t *mask;           // [n_total]
};
__global__ void __launch_bounds__(SCENE_BLOCK) select_scenes_kernel(SelectScenesArgs a)
{
    __shared__ int red[SCENE_WAVES];
    __shared__ long long best_w[SCENE_WAVES];
    __shared__ int cert_w[SCENE_WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    const int64_t g0 = f * a.n_hyp;
    // (count, index) packed so that a plain max picks the highest count and, among equals, the LOWEST index
    long long best = -1;
    int cert = 0;
    for (int h = threadIdx.x; h < a.n_hyp; h += SCENE_BLOCK) {
        const long long key = ((long long)a.count[g0 + h] << 32) | (long long)(0x7fffffff - h);
        best = key > best ? key : best;
        cert += a.status[g0 + h] == 0 ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long ob = __shfl_down(best, o);
        best = ob > best ? ob : best;
        cert += __shfl_down(cert, o);
    }
    if ((threadIdx.x & 63) == 0) { best_w[threadIdx.x >> 6] = best; cert_w[threadIdx.x >> 6] = cert; }
    __syncthreads();
    best = best_w[0]; cert = cert_w[0];
#pragma unroll
    for (int wv = 1; wv < SCENE_WAVES; ++wv) { best = best_w[wv] > best ? best_w[wv] : best; cert += cert_w[wv]; }
    int hb = (int)(0x7fffffffLL - (best & 0xffffffffLL));
    hb = hb < 0 || hb >= a.n_hyp ? 0 : hb; // (a negative count cannot win; a corrupt one must not index outside the scene's hypotheses)
    const int64_t gb = g0 + hb;
    const Slice sl = scene_slice(a.off, f, a.n_total);
    Camera cam;
    camera_load(a.R + gb * 9, a.t + gb * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const int n_inl = block_inliers(cam, sl.n, a.s2 + sl.beg * 2, a.s3 + sl.beg * 3, a.thresh * a.thresh, a.mask + sl.beg, red);
    if (threadIdx.x < 9) a.out_R[f * 9 + threadIdx.x] = a.R[gb * 9 + threadIdx.x];
    if (threadIdx.x < 3) a.out_t[f * 3 + threadIdx.x] = a.t[gb * 3 + threadIdx.x];
    if (threadIdx.x == 0) { a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = hb; a.head[f * 4 + 3] = cert; }
}

// ---- consensus assembly: ONE wavefront per scene.  (cvxpnpl_assemble_subsets gives a subset to one lane, which streams the scene
// serially: the wrong shape for a few hundred scenes of 10^3 correspondences.)  The lanes stride over the scene's correspondences, each
// with Gram sums of its own; the sums meet in a fixed-order XOR butterfly, after which every lane holds the same total -- the result
// does not depend on anything but the inputs.  The centre of the sums is the median of the subset's own first three selected records
// (cvxas::centre; any centre is exact).  Fewer than three selected: NaN, as cvx::assemble reports a singular N^T N.  The centre, the
// butterfly, the finish and the store are ransac_assemble_core.h: the LO assemblies follow the same ones.
struct ConsensusArgs {
    int64_t n_scenes, n_total;
    const int64_t *off;
    const double *s2, *s3;
    const uint8_t *mask;     // [n_total]
    const double *K;
    int32_t K_per_scene;
    double *B27, *Q45;       // [n_scenes][27], [n_scenes][45]
    int32_t *count;          // [n_scenes]
};
__global__ void __launch_bounds__(64) assemble_consensus_kernel(ConsensusArgs a)
{
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    const int lane = threadIdx.x;
    const Slice sl = scene_slice(a.off, f, a.n_total);
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    const uint8_t *mk = a.mask + sl.beg;
    double Kc[9], Ki[9], det;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = a.K[(a.K_per_scene ? f * 9 : 0) + i];
    cvx::inv3(Kc, Ki, det);
    int first[3] = {0, 0, 0}; // the first three selected correspondences, in scene order (wave-uniform)
    const int nf = cvxas::wave_first(sl.n, 3, first, [&](int64_t m) { return mk[m] != 0; });
    double c[3];
    cvxas::centre(nf, first, s3, c);
    cvx::Gram g;
    cvx::gram_zero(g);
    int n = 0;
    for (int m = lane; m < sl.n; m += 64) {
        if (!mk[m]) continue;
        cvx::gram_add_point(g, Ki, s2[2 * m], s2[2 * m + 1], s3[3 * m] - c[0], s3[3 * m + 1] - c[1], s3[3 * m + 2] - c[2]);
        ++n;
    }
    cvxas::wave_butterfly(g, n);
    double B[27], Q9[45];
    const bool ok = cvxas::finish(g, n, det, c, B, Q9);
    if (lane == 0) cvxas::store_cost(ok, B, Q9, n, f, a.B27, a.Q45, a.count); // (every lane holds the same values)
}

// ---- refit update: ONE workgroup per scene, the rule of cvxs::refit_update_kernel.  The refitted pose of the scene's consensus set is
// scored against the scene and TAKEN -- pose, status, mask and count together -- when it is usable (status 0 or 2, fitted to at least
// four correspondences) and keeps at least the consensus it was fitted to; otherwise everything of the scene stays.
struct RefitScenesArgs {
    int64_t n_scenes, n_total;
    const int64_t *off;
    const double *fit_R, *fit_t;   // [n_scenes][9], [n_scenes][3]
    const int32_t *fit_status;     // [n_scenes]
    const int32_t *fit_cnt;        // [n_scenes] size of the set each was fitted to
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *io_R, *io_t;
    int32_t *head;                 // [n_scenes][4]
    uint8_t *mask;                 // [n_total]
};
__global__ void __launch_bounds__(SCENE_BLOCK) refit_update_scenes_kernel(RefitScenesArgs a)
{
    __shared__ int red[SCENE_WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    const Slice sl = scene_slice(a.off, f, a.n_total);
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    Camera cam;
    camera_load(a.fit_R + f * 9, a.fit_t + f * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const double th2 = a.thresh * a.thresh;
    const int st = a.fit_status[f];
    const int n_new = block_inliers(cam, sl.n, s2, s3, th2, nullptr, red);
    const bool take = (st == 0 || st == 2) && a.fit_cnt[f] >= 4 && n_new >= a.head[f * 4 + 1]; // (workgroup-uniform)
    __syncthreads();
    if (!take) return;
    (void)block_inliers(cam, sl.n, s2, s3, th2, a.mask + sl.beg, red); // pose and mask change together
    take_pose(a.fit_R, a.fit_t, f, a.io_R, a.io_t, f);
    if (threadIdx.x == 0) { a.head[f * 4] = st; a.head[f * 4 + 1] = n_new; }
}

} // namespace cvxn
