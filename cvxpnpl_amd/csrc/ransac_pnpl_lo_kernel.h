// ransac_pnpl_lo_kernel.h -- local optimisation in adaptive RANSAC over points AND lines (include/cvxpnpl_amd_ransac_pnpl_lo.h, DESIGN.md
// section 25): at the end of a round every active scene's running best is refitted on the points and lines within the step's threshold
// of it, and the refitted pose's inlier count -- points plus lines -- drives the stopping rule.  Two kernels around the solve at the cost
// seam, both in the COMPACT layout of a round (entry a of the active list; an entry outside [0, n_scenes) is skipped, not clamped) over
// the clamped slices of cvxnl::scene_of.  The rules are ransac_pnpl_lo_core.h, ransac_lo_core.h and ransac_assemble_core.h; the camera,
// the predicates and the masks of a pose are cvxn::camera_load, cvxn::is_inlier, cvxnl::is_line_inlier and cvxnl::block_inliers as they
// stand.  Every loop is bounded by P_f, L_f or a constant; nothing waits for another workgroup; no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_adaptive_core.h"
#include "ransac_common.h"
#include "ransac_lo_core.h"
#include "ransac_pnpl_common.h"
#include "ransac_pnpl_lo_core.h"

namespace cvxnllo {

using cvxas::wave_uniform;
using cvxn::SCENE_BLOCK;
using cvxn::SCENE_WAVES;
using cvxnl::Scene;
using cvxnl::SceneSet;

// positions of the first `want` (at most 3) of n correspondences that pass pred(m), in scene order, by chunks of LANES: a wavefront
// ballots its 64 lanes, the four ballots meet in LDS, and a taken correspondence whose rank -- those found in earlier chunks, the
// earlier waves' (in wave order) and the earlier lanes' of its own wave -- is below `want` writes its position into slot[rank].  Every
// lane of the workgroup calls it (barriers) and gets the same answer, in scalar registers.
template <class Pred>
__device__ inline int first_taken(int n, int want, int *first, unsigned long long *ballot_w /* LDS, WAVES */, int *slot /* LDS, 3 */, Pred pred)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nf = 0;
    for (int64_t base = 0; base < n && nf < want; base += LANES) {
        const int64_t m = base + tid;
        const bool in = m < n && pred(m);
        const unsigned long long b = __ballot(in);
        __syncthreads(); // (the ballots of the chunk before have been read)
        if (lane == 0) ballot_w[wave] = b;
        __syncthreads();
        int before = nf, tot = nf;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int cw = __popcll(ballot_w[w]);
            before += w < wave ? cw : 0;
            tot += cw;
        }
        const int rank = before + __popcll(b & ((1ull << lane) - 1ull));
        if (in && rank < want) slot[rank] = (int)m; // (< n; rank < want <= 3)
        nf = __builtin_amdgcn_readfirstlane(tot < want ? tot : want);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) first[k] = k < nf ? __builtin_amdgcn_readfirstlane(slot[k]) : 0;
    return nf;
}

// ---- the assembly of a step: ONE workgroup of four wavefronts per active entry.  cvxnl::assemble_consensus_kernel with the two inlier
// predicates in place of the two masks: the points and lines that pass them at the scene's running pose (R[f], t[f]) under thresh_k are
// summed into the cost (B27, Q45)[a] of the entry; count[a] is their number, a line counting once.  The kernel reads no mask and writes
// none.  A lane keeps 60 sums over its stride of the scene's points and then of its lines; a wavefront adds its lanes in a fixed-order
// XOR butterfly; the four wave sums meet in LDS in wave order; wavefront 0 finishes from the totals in LDS, so that the sums of the loops
// and B, Q of the finish are never live together.  The result depends on the inputs alone.  Fewer than three taken: NaN, with the count
// reported.
struct LoAssembleArgs {
    SceneSet s;
    int64_t n_active;
    const int32_t *active;
    const double *R, *t;     // [n_scenes][9], [n_scenes][3]: the running poses
    double thresh_k;         // thresh * m_k
    double *B27, *Q45;       // [n_active][27], [n_active][45]
    int32_t *count;          // [n_active]
};
__global__ void __launch_bounds__(LANES) lo_assemble_pnpl_active_kernel(LoAssembleArgs a)
{
    __shared__ double part[WAVES * GRAM];
    __shared__ double total[GRAM];
    __shared__ unsigned long long ballot_w[WAVES];
    __shared__ int cnt_w[WAVES];
    __shared__ int slot[3];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.s.n_scenes) return; // (block-uniform) skipped, not clamped
    const int tid = threadIdx.x;
    const Scene sc = scene(a.s, f);
    cvxn::Camera cam;
    cvxnlo::camera(a.R + f * 9, a.t + f * 3, sc.K, cam);
    wave_uniform(cam.M);
    wave_uniform(cam.r2);
    cam.t2 = wave_uniform(cam.t2);
    const double th = a.thresh_k, th2 = a.thresh_k * a.thresh_k;
    // the first three taken records: up to three points, then -- while fewer than three records -- up to two lines (block-uniform)
    int fp[3] = {0, 0, 0}, fl[3] = {0, 0, 0};
    const int nfp = first_taken(sc.P, 3, fp, ballot_w, slot, [&](int64_t m) { return cvxnlo::taken(cam, sc.p2, sc.p3, m, th2); });
    const int nfl = first_taken(sc.L, cvxas::centre_lines_wanted(nfp), fl, ballot_w, slot, [&](int64_t m) { return line_taken(cam, sc.l2, sc.l3, m, th); });
    double c[3];
    cvxas::centre(nfp, fp, nfl, fl, sc.p3, sc.l3, c);
    wave_uniform(c);
    double Kc[9], Ki[9], det; // (K^-1 only now: the search above holds enough in scalar registers without it)
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = sc.K[i];
    cvx::inv3(Kc, Ki, det);
    wave_uniform(Ki);
    cvx::Gram g;
    int n = lane_sums(tid, sc, cam, th, th2, Ki, c, g);
    cvxas::wave_butterfly(g, n);
    cvxas::block_finish_store(g, n, part, total, cnt_w, det, c, ai, a.B27, a.Q45, a.count);
}

// ---- the update of a step: ONE workgroup per active entry, cvxnlo::lo_update_active_kernel over a cvxnl::Scene.  The refitted pose
// (fit_R, fit_t, fit_status)[a] is scored against scene f = active[a] at thresh over its points and lines -- counting first; the two
// masks are written only when the pose is taken -- and TAKEN under cvxnlo::take_fit; then pose, head[f][0..1], best[f] and the scene's
// slices of both masks change together, head[f][2] keeps the index of the hypothesis that seeded the fit, and lo_taken[f] goes up by
// one.  Taken or not, done[a] |= scene_done at the scene's best over P_f + L_f: a flag that is set stays set.
struct LoUpdateArgs {
    SceneSet s;
    int64_t n_active;
    int32_t cap;
    double confidence;
    const int32_t *active;
    const double *fit_R, *fit_t;   // [n_active][9], [n_active][3]
    const int32_t *fit_status;     // [n_active]
    const int32_t *fit_cnt;        // [n_active] size of the set each was fitted to
    double thresh;
    double *io_R, *io_t;           // [n_scenes][9], [n_scenes][3]
    int32_t *head;                 // [n_scenes][4]
    int32_t *best;                 // [n_scenes]
    uint8_t *mask_p, *mask_l;      // [n_pts], [n_lines]
    const int32_t *hyp_used;       // [n_scenes]
    int32_t *lo_taken;             // [n_scenes]
    int32_t *done;                 // [n_active]
};
__global__ void __launch_bounds__(SCENE_BLOCK) lo_update_pnpl_active_kernel(LoUpdateArgs a)
{
    __shared__ int red[SCENE_WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.s.n_scenes) return; // (block-uniform) skipped, not clamped
    const Scene sc = cvxnl::scene_of(a.s, f);
    cvxn::Camera cam;
    cvxn::camera_load(a.fit_R + ai * 9, a.fit_t + ai * 3, sc.K, cam);
    const int st = a.fit_status[ai];
    const int best_prev = a.best[f], head_prev = a.head[f * 4 + 1]; // (every lane reads both before lane 0 stores: barriers between)
    const int n_new = cvxnl::block_inliers(cam, sc, a.thresh, nullptr, nullptr, red);
    const bool take = cvxnlo::take_fit(st, a.fit_cnt[ai], n_new, best_prev, head_prev); // (workgroup-uniform)
    __syncthreads();
    if (take) (void)cvxnl::block_inliers(cam, sc, a.thresh, a.mask_p + sc.beg_p, a.mask_l + sc.beg_l, red); // pose and masks change together
    cvxnlo::commit_fit(take, st, n_new, best_prev, sc.P + sc.L, a.fit_R, a.fit_t, ai, a.io_R, a.io_t, f, a.head, a.best, a.lo_taken, a.hyp_used, a.cap,
                       a.confidence, a.done);
}

} // namespace cvxnllo
