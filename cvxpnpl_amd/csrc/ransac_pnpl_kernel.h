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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxnl {

using cvxn::Camera;
using cvxn::Slice;

constexpr int BLOCK = 256;       // lanes of the sampling / scoring / selection / refit workgroups
constexpr int WAVES = BLOCK / 64;
constexpr int POINT_TILE = 512;  // points per LDS tile of the scoring kernel: 5 doubles each (20 KB)
constexpr int LINE_TILE = 256;   // lines per LDS tile: 9 doubles each (18 KB), in the same buffer
constexpr int TILE_DOUBLES = POINT_TILE * 5;
static_assert(LINE_TILE * 9 <= TILE_DOUBLES && LINE_TILE <= BLOCK, "a line tile fits the buffer and is staged one line per lane");

// the scene set every kernel sees
struct SceneSet {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l;  // [n_scenes + 1] each
    const double *p2, *p3;         // [n_pts][2], [n_pts][3]
    const double *l2, *l3;         // [n_lines][4] (u0 v0 u1 v1), [n_lines][6] (P0 P1)
    const double *K;               // [9] or [n_scenes][9]
    int32_t K_per_scene;
};
struct Scene {
    int32_t P, L;                  // L is cut so that P + L fits an int32
    const double *p2, *p3, *l2, *l3;
    int64_t beg_p, beg_l;
    const double *K;
};
__device__ inline Scene scene_of(const SceneSet &s, int64_t f)
{
    const Slice sp = cvxn::scene_slice(s.off_p, f, s.n_pts), sl = cvxn::scene_slice(s.off_l, f, s.n_lines);
    Scene sc;
    sc.P = sp.n;
    sc.L = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    sc.beg_p = sp.beg; sc.beg_l = sl.beg;
    sc.p2 = s.p2 + sp.beg * 2; sc.p3 = s.p3 + sp.beg * 3; // (never followed where P or L is 0)
    sc.l2 = s.l2 + sl.beg * 4; sc.l3 = s.l3 + sl.beg * 6;
    sc.K = s.K + (s.K_per_scene ? f * 9 : 0);
    return sc;
}

// ---- the line inlier predicate, beside cvxn::is_inlier for points: ONE statement of it, used by the scoring kernel (counts) and by the
// workgroup kernels (masks).  A 2D line is two pixel samples a, b on it; the image line is l = (a, 1) x (b, 1), and l . (u, v, 1) /
// hypot(l_0, l_1) is the signed distance of pixel (u, v) from it.  A line is an inlier of a pose when BOTH 3D end points have depth > 0
// and BOTH projected end points lie within thresh pixels of the image line.  image_line normalises l once (the scoring kernel does it
// once per tile); a degenerate line (a = b) has hypot = 0 and gets l_0 = 0 * inf = NaN, so it compares false under every pose, as a NaN
// pose does on every line.
__device__ inline void image_line(double ax, double ay, double bx, double by, double *l)
{
    const double l0 = ay - by, l1 = bx - ax, l2 = ax * by - ay * bx;
    const double inv = 1.0 / hypot(l0, l1);
    l[0] = l0 * inv; l[1] = l1 * inv; l[2] = l2 * inv;
}
__device__ inline bool end_point_near(const Camera &c, const double *l, double X, double Y, double Z, double thresh)
{
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double d = l[0] * (u / w) + l[1] * (v / w) + l[2];
    return depth > 0.0 && (fabs(d) < thresh);
}
__device__ inline bool is_line_inlier_normalised(const Camera &c, const double *l /* image_line */, const double *e /* P0 P1 */, double thresh)
{
    return end_point_near(c, l, e[0], e[1], e[2], thresh) && end_point_near(c, l, e[3], e[4], e[5], thresh);
}
__device__ inline bool is_line_inlier(const Camera &c, const double *ab /* u0 v0 u1 v1 */, const double *e /* P0 P1 */, double thresh)
{
    double l[3];
    image_line(ab[0], ab[1], ab[2], ab[3], l);
    return is_line_inlier_normalised(c, l, e, thresh);
}

// ---- sampling and minimal assembly: one lane per (scene, hypothesis), grid (ceil(H / 256), scenes).  The draw is that of
// cvxn::sample_scenes_kernel over M_f = P_f + L_f (cvxn::draw_minimal_set: same key, same counter); index c < P_f is point c, otherwise
// line c - P_f.  The lane assembles its set in place, in the order and about the centre cvxa / cvx::assemble use on the gathered set:
// points in draw order, then lines in draw order; centre = cvx::shift_centre of the first three 3D records in that order (a set of four
// correspondences always has at least four records).  Q45 and B27 feed cvxpnpl_solve_cost_batch.
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
    const int32_t M = sc.P + sc.L;
    const int64_t g = f * a.n_hyp + h;
    double Kc[9], Ki[9], det;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = sc.K[i];
    cvx::inv3(Kc, Ki, det);
    const bool drawable = M >= 4 && (det == det) && det != 0.0; // what idx reports: apart from what gram_finish finds in the set itself
    int pick[4] = {-1, -1, -1, -1};
    double c[3] = {0.0, 0.0, 0.0};
    cvx::Gram gm;
    cvx::gram_zero(gm);
    if (M >= 4) {
        cvxn::draw_minimal_set(M, a.seed[f], (uint32_t)h, pick); // 0 .. M - 1 by construction
        // the first three 3D records of the set: its points in draw order, then the end points of its lines in draw order
        double first3[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int nrec = 0;
        auto put = [&](const double *r) { // (static indices: registers)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                first3[k] = nrec == 0 ? r[k] : first3[k];
                first3[3 + k] = nrec == 1 ? r[k] : first3[3 + k];
                first3[6 + k] = nrec == 2 ? r[k] : first3[6 + k];
            }
            ++nrec;
        };
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pick[j] < sc.P) put(sc.p3 + 3 * (int64_t)pick[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pick[j] >= sc.P && nrec < 3) {
                const double *e = sc.l3 + 6 * (int64_t)(pick[j] - sc.P);
                put(e);
                put(e + 3);
            }
        cvx::shift_centre(3, first3, 0, nullptr, c);
#pragma unroll 1
        for (int j = 0; j < 4; ++j) { // (rolled: one copy of the 60 accumulations per kind)
            const int q = j == 0 ? pick[0] : (j == 1 ? pick[1] : (j == 2 ? pick[2] : pick[3]));
            if (q < sc.P) {
                const double *x = sc.p2 + 2 * (int64_t)q, *X = sc.p3 + 3 * (int64_t)q;
                cvx::gram_add_point(gm, Ki, x[0], x[1], X[0] - c[0], X[1] - c[1], X[2] - c[2]);
            }
        }
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int q = j == 0 ? pick[0] : (j == 1 ? pick[1] : (j == 2 ? pick[2] : pick[3]));
            if (q >= sc.P) {
                const double *x = sc.l2 + 4 * (int64_t)(q - sc.P), *e = sc.l3 + 6 * (int64_t)(q - sc.P);
                const double ab[4] = {x[0], x[1], x[2], x[3]};
                const double es[6] = {e[0] - c[0], e[1] - c[1], e[2] - c[2], e[3] - c[0], e[4] - c[1], e[5] - c[2]};
                cvx::gram_add_line(gm, Ki, ab, es);
            }
        }
    }
    double B[27], Q9[45];
    const bool ok = cvx::gram_finish(gm, B, Q9) && drawable;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j]; // t = -B' r - R c
    if (a.idx) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a.idx[g * 4 + j] = drawable ? pick[j] : -1; // fewer than four correspondences or a singular K: no set
    }
#pragma unroll
    for (int i = 0; i < 27; ++i) a.B27[g * 27 + i] = ok ? B[i] : NAN;
#pragma unroll
    for (int i = 0; i < 45; ++i) a.Q45[g * 45 + i] = ok ? Q9[i] : NAN;
}

// ---- scoring: grid (ceil(H / 256), scenes), one lane per hypothesis of the workgroup's scene.  The scene's points go through LDS a tile
// at a time and are broadcast to the lanes, as in cvxn::score_scenes_kernel; then its lines, a tile of end points plus the NORMALISED
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
    bool usable = live;
    if (live && a.status) {
        const int32_t s = a.status[g];
        usable = s >= 0 && s < 32 && ((a.usable_mask >> s) & 1u);
    }
    const double th2 = a.thresh * a.thresh;
    int cnt = 0;
    for (int64_t base = 0; base < sc.P; base += POINT_TILE) {
        const int n = sc.P - base < POINT_TILE ? (int)(sc.P - base) : POINT_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            const int64_t m = base + i;
            tile[i * 5 + 0] = sc.p3[m * 3 + 0];
            tile[i * 5 + 1] = sc.p3[m * 3 + 1];
            tile[i * 5 + 2] = sc.p3[m * 3 + 2];
            tile[i * 5 + 3] = sc.p2[m * 2 + 0];
            tile[i * 5 + 4] = sc.p2[m * 2 + 1];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            cnt += usable && cvxn::is_inlier(cam, tile[i * 5], tile[i * 5 + 1], tile[i * 5 + 2], tile[i * 5 + 3], tile[i * 5 + 4], th2) ? 1 : 0;
    }
    for (int64_t base = 0; base < sc.L; base += LINE_TILE) {
        const int n = sc.L - base < LINE_TILE ? (int)(sc.L - base) : LINE_TILE;
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const int64_t m = base + (int)threadIdx.x;
            const int i = threadIdx.x;
#pragma unroll
            for (int k = 0; k < 6; ++k) tile[i * 9 + k] = sc.l3[m * 6 + k];
            double l[3];
            image_line(sc.l2[m * 4], sc.l2[m * 4 + 1], sc.l2[m * 4 + 2], sc.l2[m * 4 + 3], l);
            tile[i * 9 + 6] = l[0]; tile[i * 9 + 7] = l[1]; tile[i * 9 + 8] = l[2];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            cnt += usable && is_line_inlier_normalised(cam, tile + i * 9 + 6, tile + i * 9, a.thresh) ? 1 : 0;
    }
    if (live) a.count[g] = cnt;
}

// inliers of ONE pose over one scene's points and lines, by the lanes of one workgroup: writes both masks (optional, together) and returns
// points + lines to every lane
__device__ inline int block_inliers(const Camera &cam, const Scene &sc, double thresh, uint8_t *mask_p, uint8_t *mask_l, int *red /* LDS, WAVES ints */)
{
    const double th2 = thresh * thresh;
    int cnt = 0;
    for (int64_t m = threadIdx.x; m < sc.P; m += BLOCK) { // (int64: m + BLOCK may pass 2^31 where P_f is within a stride of it)
        const bool in = cvxn::is_inlier(cam, sc.p3[3 * m], sc.p3[3 * m + 1], sc.p3[3 * m + 2], sc.p2[2 * m], sc.p2[2 * m + 1], th2);
        cnt += in ? 1 : 0;
        if (mask_p) mask_p[m] = in ? 1 : 0;
    }
    for (int64_t m = threadIdx.x; m < sc.L; m += BLOCK) {
        const double *x = sc.l2 + 4 * m, *e = sc.l3 + 6 * m;
        const double ab[4] = {x[0], x[1], x[2], x[3]}, es[6] = {e[0], e[1], e[2], e[3], e[4], e[5]};
        const bool in = is_line_inlier(cam, ab, es, thresh);
        cnt += in ? 1 : 0;
        if (mask_l) mask_l[m] = in ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) tot += red[wv];
    return tot;
}

// ---- selection: ONE workgroup per scene, cvxn::select_scenes_kernel with two masks.  Arg-max of the scene's H counts with the LOWEST
// index winning a tie, the number of certified hypotheses on the way, then the winner's pose and -- scored again by the workgroup's
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
    __shared__ int red[WAVES];
    __shared__ long long best_w[WAVES];
    __shared__ int cert_w[WAVES];
    const int64_t f = blockIdx.x;
    if (f >= a.s.n_scenes) return;
    const int64_t g0 = f * a.n_hyp;
    // (count, index) packed so that a plain max picks the highest count and, among equals, the LOWEST index
    long long best = -1;
    int cert = 0;
    for (int64_t h = threadIdx.x; h < a.n_hyp; h += BLOCK) {
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
    for (int wv = 1; wv < WAVES; ++wv) { best = best_w[wv] > best ? best_w[wv] : best; cert += cert_w[wv]; }
    int hb = (int)(0x7fffffffLL - (best & 0xffffffffLL));
    hb = hb < 0 || hb >= a.n_hyp ? 0 : hb; // (a negative count cannot win; a corrupt one must not index outside the scene's hypotheses)
    const int64_t gb = g0 + hb;
    const Scene sc = scene_of(a.s, f);
    Camera cam;
    cvxn::camera_load(a.R + gb * 9, a.t + gb * 3, sc.K, cam);
    const int n_inl = block_inliers(cam, sc, a.thresh, a.mask_p + sc.beg_p, a.mask_l + sc.beg_l, red);
    if (threadIdx.x < 9) a.out_R[f * 9 + threadIdx.x] = a.R[gb * 9 + threadIdx.x];
    if (threadIdx.x < 3) a.out_t[f * 3 + threadIdx.x] = a.t[gb * 3 + threadIdx.x];
    if (threadIdx.x == 0) { a.head[f * 4] = a.status[gb]; a.head[f * 4 + 1] = n_inl; a.head[f * 4 + 2] = hb; a.head[f * 4 + 3] = cert; }
}

// ---- consensus assembly: ONE wavefront per scene, cvxn::assemble_consensus_kernel over masked points, then masked lines.  The lanes
// stride over the scene's correspondences, each with Gram sums of its own; the 60 sums meet in a fixed-order XOR butterfly, after which
// every lane holds the same total: the result depends on the inputs only.  The centre is cvx::shift_centre of the first three selected
// 3D RECORDS in the order "points, then lines" (a line contributes its two end points): the centre cvxpnpl_assemble_batch uses on the
// gathered set.  Fewer than three CORRESPONDENCES taken, a singular N^T N or a singular K: NaN for that scene only.
struct ConsensusArgs {
    SceneSet s;
    const uint8_t *mask_p, *mask_l;  // [n_pts], [n_lines]
    double *B27, *Q45;               // [n_scenes][27], [n_scenes][45]
    int32_t *count;                  // [n_scenes]
};
__device__ inline double wave_xor_add(double v, int o) { return v + __shfl_xor(v, o); }
// positions of the first `want` (at most 3) set entries of mask[0 .. n), in order: ballots over chunks of 64 (wave-uniform)
__device__ inline int first_selected(const uint8_t *mask, int n, int want, int *first)
{
    const int lane = threadIdx.x;
    int nf = 0;
    for (int64_t base = 0; base < n && nf < want; base += 64) {
        const int64_t m = base + lane;
        unsigned long long b = __ballot(m < n && mask[m] != 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (b != 0 && nf < want) {
                const int pos = (int)base + __ffsll((long long)b) - 1; // (< n)
                first[0] = nf == 0 ? pos : first[0]; first[1] = nf == 1 ? pos : first[1]; first[2] = nf == 2 ? pos : first[2];
                ++nf;
                b &= b - 1;
            }
        }
    }
    return nf;
}
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
    const int nfp = first_selected(mp, sc.P, 3, fp);
    const int nfl = nfp < 3 ? first_selected(ml, sc.L, nfp == 0 ? 2 : 1, fl) : 0;
    const int nrec = nfp + 2 * nfl < 3 ? nfp + 2 * nfl : 3;
    double c[3] = {0.0, 0.0, 0.0};
    if (nrec > 0) {
        double first3[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) { // (entries beyond nrec repeat the first record and are not read by shift_centre)
            const int kk = k < nrec ? k : 0;
            const double *r;
            if (kk < nfp) {
                r = sc.p3 + 3 * (int64_t)(kk == 0 ? fp[0] : (kk == 1 ? fp[1] : fp[2]));
            } else {
                const int e = kk - nfp; // end point e of the selected lines: line e / 2, end e % 2
                r = sc.l3 + 6 * (int64_t)(e < 2 ? fl[0] : fl[1]) + 3 * (e & 1);
            }
            first3[3 * k] = r[0]; first3[3 * k + 1] = r[1]; first3[3 * k + 2] = r[2];
        }
        cvx::shift_centre(nrec, first3, 0, nullptr, c);
    }
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
#pragma unroll 1
    for (int o = 1; o < 64; o <<= 1) { // (rolled: six passes over the same 60 sums)
#pragma unroll
        for (int i = 0; i < 6; ++i) g.M0[i] = wave_xor_add(g.M0[i], o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 6; ++i) g.M1[k][i] = wave_xor_add(g.M1[k][i], o);
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < 6; ++i) g.M2[k][i] = wave_xor_add(g.M2[k][i], o);
        n += __shfl_xor(n, o);
    }
    double B[27], Q9[45];
    const bool ok = n >= 3 && cvx::gram_finish(g, B, Q9) && (det == det) && det != 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j];
    if (lane == 0) { // (every lane holds the same values; static indices keep B and Q9 in registers)
#pragma unroll
        for (int i = 0; i < 27; ++i) a.B27[f * 27 + i] = ok ? B[i] : NAN;
#pragma unroll
        for (int i = 0; i < 45; ++i) a.Q45[f * 45 + i] = ok ? Q9[i] : NAN;
        a.count[f] = n;
    }
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
    __shared__ int red[WAVES];
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
    if (threadIdx.x < 9) a.io_R[f * 9 + threadIdx.x] = a.fit_R[f * 9 + threadIdx.x];
    if (threadIdx.x < 3) a.io_t[f * 3 + threadIdx.x] = a.fit_t[f * 3 + threadIdx.x];
    if (threadIdx.x == 0) { a.head[f * 4] = st; a.head[f * 4 + 1] = n_new; }
}

} // namespace cvxnl
