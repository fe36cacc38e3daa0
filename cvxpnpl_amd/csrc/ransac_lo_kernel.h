// ransac_lo_kernel.h -- local optimisation in adaptive RANSAC (include/cvxpnpl_amd_ransac_lo.h): at the end of a
// round every active scene's running best is refitted on its consensus set by the non-minimal solver, and the refitted pose's inlier
// count drives the stopping rule.  Two kernels around the solve at the cost seam, both in the COMPACT layout of a round (entry a of the
// active list; an entry outside [0, n_scenes) is skipped, not clamped) over the clamped slices of cvxn::scene_slice, and one that zeroes
// the counter.  The rules are ransac_lo_core.h and ransac_assemble_core.h; the camera, the predicate and the mask of a pose are cvxn::camera_load, cvxn::is_inlier
// and cvxn::block_inliers as they stand.  Every loop is bounded by M_f or a constant; nothing waits for another workgroup; no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_adaptive_core.h"
#include "ransac_common.h"
#include "ransac_lo_core.h"

namespace cvxnlo {

using cvxas::wave_uniform;
using cvxn::SCENE_BLOCK;
using cvxn::SCENE_WAVES;

// ---- the assembly of a step: ONE workgroup of four wavefronts per active entry.  cvxn::assemble_consensus_kernel with the inlier
// predicate in place of the mask: the correspondences that pass it at the scene's running pose (R[f], t[f]) under thresh_k are summed
// into the cost (B27, Q45)[a] of the entry; count[a] is their number.  The kernel reads no mask and writes none.  A lane keeps 60 sums
// over its stride of the scene; a wavefront adds its lanes in a fixed-order XOR butterfly; the four wave sums meet in LDS in wave order;
// wavefront 0 finishes from the totals in LDS, so that the sums of the loop and B, Q of the finish are never live together.  The result
// depends on the inputs alone.  Fewer than three taken: NaN, with the count reported.
struct LoAssembleArgs {
    int64_t n_active, n_scenes, n_total;
    const int32_t *active;
    const int64_t *off;
    const double *s2, *s3;
    const double *R, *t;     // [n_scenes][9], [n_scenes][3]: the running poses
    const double *K;         // [9] or [n_scenes][9]
    int32_t K_per_scene;
    double thresh_k;         // thresh * m_k
    double *B27, *Q45;       // [n_active][27], [n_active][45]
    int32_t *count;          // [n_active]
};
__global__ void __launch_bounds__(LANES) lo_assemble_active_kernel(LoAssembleArgs a)
{
    __shared__ double part[WAVES * GRAM];
    __shared__ double total[GRAM];
    __shared__ unsigned long long ballot_w[WAVES];
    __shared__ int cnt_w[WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform) skipped, not clamped
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    double Kc[9], Ki[9], det;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = a.K[(a.K_per_scene ? f * 9 : 0) + i];
    cvx::inv3(Kc, Ki, det);
    cvxn::Camera cam;
    camera(a.R + f * 9, a.t + f * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    wave_uniform(Ki);
    wave_uniform(cam.M);
    wave_uniform(cam.r2);
    cam.t2 = wave_uniform(cam.t2);
    const double th2 = a.thresh_k * a.thresh_k;
    // the first three taken correspondences, in scene order: ballots over chunks of LANES, the four waves' in wave order (block-uniform)
    int first[3] = {0, 0, 0}, nf = 0;
    for (int base = 0; base < sl.n && nf < 3; base += LANES) {
        const int m = base + tid;
        const unsigned long long b = __ballot(m < sl.n && taken(cam, s2, s3, m, th2));
        __syncthreads(); // (the ballots of the chunk before have been read)
        if (lane == 0) ballot_w[wave] = b;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            unsigned long long bw = ballot_w[w];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (bw != 0 && nf < 3) {
                    const int pos = base + w * 64 + __ffsll((long long)bw) - 1;
                    first[0] = nf == 0 ? pos : first[0]; first[1] = nf == 1 ? pos : first[1]; first[2] = nf == 2 ? pos : first[2];
                    ++nf;
                    bw &= bw - 1;
                }
            }
        }
    }
    double c[3];
    cvxas::centre(nf, first, s3, c);
    wave_uniform(c);
    cvx::Gram g;
    int n = lane_sums(tid, sl.n, s2, s3, cam, th2, Ki, c, g);
    cvxas::wave_butterfly(g, n);
    cvxas::block_finish_store(g, n, part, total, cnt_w, det, c, ai, a.B27, a.Q45, a.count);
}

// ---- the update of a step: ONE workgroup per active entry.  The refitted pose (fit_R, fit_t, fit_status)[a] is scored against scene
// f = active[a] at thresh -- counting first; the mask is written only when the pose is taken -- and TAKEN under take_fit; then pose,
// head[f][0..1], best[f] and the scene's slice of the mask change together, head[f][2] keeps the index of the hypothesis that seeded
// the fit, and lo_taken[f] goes up by one.  Taken or not, done[a] |= scene_done at the scene's best: a flag that is set stays set.
struct LoUpdateArgs {
    int64_t n_active, n_scenes, n_total;
    int32_t cap;
    double confidence;
    const int32_t *active;
    const int64_t *off;
    const double *fit_R, *fit_t;   // [n_active][9], [n_active][3]
    const int32_t *fit_status;     // [n_active]
    const int32_t *fit_cnt;        // [n_active] size of the set each was fitted to
    const double *K;
    int32_t K_per_scene;
    const double *s2, *s3;
    double thresh;
    double *io_R, *io_t;           // [n_scenes][9], [n_scenes][3]
    int32_t *head;                 // [n_scenes][4]
    int32_t *best;                 // [n_scenes]
    uint8_t *mask;                 // [n_total]
    const int32_t *hyp_used;       // [n_scenes]
    int32_t *lo_taken;             // [n_scenes]
    int32_t *done;                 // [n_active]
};
__global__ void __launch_bounds__(SCENE_BLOCK) lo_update_active_kernel(LoUpdateArgs a)
{
    __shared__ int red[SCENE_WAVES];
    const int64_t ai = blockIdx.x;
    if (ai >= a.n_active) return;
    const int64_t f = a.active[ai];
    if (f < 0 || f >= a.n_scenes) return; // (block-uniform) skipped, not clamped
    const cvxn::Slice sl = cvxn::scene_slice(a.off, f, a.n_total);
    const double *s2 = a.s2 + sl.beg * 2, *s3 = a.s3 + sl.beg * 3;
    cvxn::Camera cam;
    cvxn::camera_load(a.fit_R + ai * 9, a.fit_t + ai * 3, a.K + (a.K_per_scene ? f * 9 : 0), cam);
    const double th2 = a.thresh * a.thresh;
    const int st = a.fit_status[ai];
    const int best_prev = a.best[f], head_prev = a.head[f * 4 + 1]; // (every lane reads both before lane 0 stores: barriers between)
    const int n_new = cvxn::block_inliers(cam, sl.n, s2, s3, th2, nullptr, red);
    const bool take = take_fit(st, a.fit_cnt[ai], n_new, best_prev, head_prev); // (workgroup-uniform)
    __syncthreads();
    if (take) (void)cvxn::block_inliers(cam, sl.n, s2, s3, th2, a.mask + sl.beg, red); // pose and mask change together
    commit_fit(take, st, n_new, best_prev, sl.n, a.fit_R, a.fit_t, ai, a.io_R, a.io_t, f, a.head, a.best, a.lo_taken, a.hyp_used, a.cap, a.confidence, a.done);
}

// ---- start of a call with local optimisation: lo_taken[f] = 0.  One lane per scene.
struct LoInitArgs {
    int64_t n_scenes;
    int32_t *lo_taken;       // [n_scenes]
};
__global__ void __launch_bounds__(SCENE_BLOCK) lo_init_kernel(LoInitArgs a)
{
    const int64_t f = (int64_t)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (f < a.n_scenes) a.lo_taken[f] = 0;
}

} // namespace cvxnlo
