// ransac_common.h -- what the five RANSAC libraries share (ransac_kernel.h, fixed budget; ransac_adaptive_kernel.h, rounds;
// ransac_guided_kernel.h, ranked draws; ransac_pnpl_kernel.h and ransac_pnpl_adaptive_kernel.h, the same over points and lines), and the
// refinement libraries for scene_slice alone (refine_view.h): steps of a scene that need only the scene, the camera and the workgroup,
// stated ONCE.  The clamped slice (scene_slice, host and device); the point inlier predicate and the mask of one pose (is_inlier,
// block_inliers); the Philox generator and the draw of a minimal set; a four-point set written as problem g (hypothesis_K,
// write_point_set, uniform_hypothesis); the usable rule and the scoring of a scene's points through LDS (hypothesis_usable,
// score_points); the arg-max of a scene's counts (block_argmax); a pose taken for a scene (take_pose).  A kernel resolves its own
// indices -- f * n_hyp + h, or the active list with its skip-not-clamp rule and the compact layout -- and then calls these with FIELDS of
// its argument block, never the block: one reference to the block changes a kernel's whole code.  score_points and block_argmax take
// the type of their loop index from the caller, so that each kernel keeps the index width it had.  No kernel here: a library that
// includes this header compiles nothing it does not launch.  (Left as copies, because the extraction changed a kernel's registers: the
// refit rule, the round bookkeeping, the point half of cvxnl::block_inliers; and the arg-max of cvxn::select_scenes_kernel -- DESIGN.md
// section 13.  The assembly of a scene subset is ransac_assemble_core.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace cvxn {

constexpr int SCENE_BLOCK = 256;  // lanes of the sampling / scoring / selection / refit workgroups
constexpr int SCENE_WAVES = SCENE_BLOCK / 64;
constexpr int POINT_TILE = 512;   // points per LDS tile of the scoring kernels: 5 doubles each (20 KB)

struct Slice { int64_t beg; int32_t n; };
__host__ __device__ inline Slice scene_slice(const int64_t *off, int64_t f, int64_t n_total)
{
    int64_t e = off[f + 1], b = off[f];
    e = e < 0 ? 0 : (e > n_total ? n_total : e);
    b = b < 0 ? 0 : (b > e ? e : b);
    const int64_t n = e - b;
    return Slice{b, (int32_t)(n > 0x7fffffffLL ? 0x7fffffffLL : n)};
}

// ---- the inlier predicate: ONE statement of it, used by the scoring kernel (counts) and by the two workgroup kernels (masks), so
// that a mask and a count cannot disagree.  The arithmetic is that of cvxs::score_kernel / cvxs::block_score_pose, expression by
// expression:  X = R P + t,  (u, v, w) = K X,  depth = X_z > 0,  |(u / w, v / w) - x|^2 < thresh^2;  a NaN pose compares false.
struct Camera {
    double M[12];      // K R | K t : pixel-space projection
    double r2[3], t2;  // depth row
};
__device__ inline void camera_load(const double *Rp, const double *tp, const double *Kp, Camera &c)
{
    double R[9], t[3], K[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = Rp[i]; K[i] = Kp[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.M[i * 4 + j] = K[i * 3] * R[j] + K[i * 3 + 1] * R[3 + j] + K[i * 3 + 2] * R[6 + j];
        c.M[i * 4 + 3] = K[i * 3] * t[0] + K[i * 3 + 1] * t[1] + K[i * 3 + 2] * t[2];
    }
    c.r2[0] = R[6]; c.r2[1] = R[7]; c.r2[2] = R[8]; c.t2 = t[2];
}
__device__ inline bool is_inlier(const Camera &c, double X, double Y, double Z, double x, double y, double th2)
{
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double du = u / w - x, dv = v / w - y;
    return depth > 0.0 && (du * du + dv * dv < th2);
}

// inliers of ONE pose over one scene, by the lanes of one workgroup: writes mask (optional) and returns the count to every lane
__device__ inline int block_inliers(const Camera &cam, int n, const double *s2, const double *s3, double th2, uint8_t *mask, int *red /* LDS, SCENE_WAVES ints */)
{
    int cnt = 0;
    for (int m = threadIdx.x; m < n; m += SCENE_BLOCK) {
        const bool in = is_inlier(cam, s3[3 * m], s3[3 * m + 1], s3[3 * m + 2], s2[2 * m], s2[2 * m + 1], th2);
        cnt += in ? 1 : 0;
        if (mask) mask[m] = in ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int wv = 0; wv < SCENE_WAVES; ++wv) tot += red[wv];
    return tot;
}

// ---- scoring, one pose per LANE.  The usable rule: a lane past the end scores nothing, nor does a status outside usable_mask (bit s
// set: status s is scored; no status array: every live hypothesis is).
__device__ inline bool hypothesis_usable(bool live, const int32_t *status, int64_t g, uint32_t usable_mask)
{
    bool usable = live;
    if (live && status) {
        const int32_t s = status[g];
        usable = s >= 0 && s < 32 && ((usable_mask >> s) & 1u);
    }
    return usable;
}
// The scene's n points go through LDS a tile at a time and are broadcast to the lanes (a ds_read of a wave-uniform address).  Every lane
// of the workgroup calls it (barriers); returns the point inliers of the lane's pose.  Index: the type of the tile base, as above.
template <class Index>
__device__ inline int score_points(double *tile /* LDS, POINT_TILE * 5 */, int n_pts, const double *s2, const double *s3, const Camera &cam, bool usable,
                                   double th2)
{
    int cnt = 0;
    for (Index base = 0; base < n_pts; base += POINT_TILE) {
        const int n = n_pts - base < POINT_TILE ? (int)(n_pts - base) : POINT_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += SCENE_BLOCK) {
            const int64_t m = base + i;
            tile[i * 5 + 0] = s3[m * 3 + 0];
            tile[i * 5 + 1] = s3[m * 3 + 1];
            tile[i * 5 + 2] = s3[m * 3 + 2];
            tile[i * 5 + 3] = s2[m * 2 + 0];
            tile[i * 5 + 4] = s2[m * 2 + 1];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            cnt += usable && is_inlier(cam, tile[i * 5], tile[i * 5 + 1], tile[i * 5 + 2], tile[i * 5 + 3], tile[i * 5 + 4], th2) ? 1 : 0;
    }
    return cnt;
}

// ---- the arg-max of the n counts count[g0 .. g0 + n) by one workgroup, the LOWEST index winning a tie, and the number of certified
// hypotheses (status 0) on the way.  (count, index) are packed so that a plain max picks the highest count and, among equals, the lowest
// index.  Every lane gets the same Winner; h is inside [0, n): a negative count cannot win, and a corrupt one must not index outside the
// scene's hypotheses.
struct Winner { int h, count, cert; };
template <class Index>
__device__ inline Winner block_argmax(const int32_t *count, const int32_t *status, int64_t g0, int n, long long *best_w, int *cert_w /* LDS, SCENE_WAVES each */)
{
    long long best = -1;
    int cert = 0;
    for (Index h = threadIdx.x; h < n; h += SCENE_BLOCK) {
        const long long key = ((long long)count[g0 + h] << 32) | (long long)(0x7fffffff - h);
        best = key > best ? key : best;
        cert += status[g0 + h] == 0 ? 1 : 0;
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
    hb = hb < 0 || hb >= n ? 0 : hb;
    return Winner{hb, (int)(best >> 32), cert};
}

// ---- a pose TAKEN for scene f by its workgroup: pose g of R / t becomes the scene's (the caller writes the mask(s) before and the head after)
__device__ inline void take_pose(const double *R, const double *t, int64_t g, double *out_R, double *out_t, int64_t f)
{
    if (threadIdx.x < 9) out_R[f * 9 + threadIdx.x] = R[g * 9 + threadIdx.x];
    if (threadIdx.x < 3) out_t[f * 3 + threadIdx.x] = t[g * 3 + threadIdx.x];
}

// ---- Philox4x32-10, the generator of every sampler (cvxs::sample_sets_kernel, sample_scenes_kernel, cvxnl::sample_assemble_kernel)
__device__ inline void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- the draw of a minimal set: four distinct indices of 0 .. n - 1 (n >= 4) by a partial Fisher-Yates on the Philox stream keyed by the
// scene's seed, counter (hypothesis index within the scene, 0, 0xFFFFFFFE, 0): what cvxs::sample_sets_kernel draws for k = 4.
__device__ inline void draw_minimal_set(int32_t n, uint64_t seed, uint32_t h, int *pick)
{
    uint32_t w[4];
    philox4x32(h, 0u, 0xFFFFFFFEu, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    int pos[4], val[4]; // positions already swapped and what sits there now (static indices: registers)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t span = (uint32_t)(n - j);
        const int r = j + (int)(((uint64_t)w[j] * span) >> 32); // uniform on j .. n - 1
        int vr = r, vj = j;
#pragma unroll
        for (int m = 0; m < j; ++m) {
            vr = pos[m] == r ? val[m] : vr;
            vj = pos[m] == j ? val[m] : vj;
        }
        pick[j] = vr;
        pos[j] = r; val[j] = vj;
#pragma unroll
        for (int m = 0; m < j; ++m) // a later entry for the same position overrides an earlier one
            if (pos[m] == r) pos[m] = -1;
    }
}

// ---- a four-point hypothesis written as problem g of the minimal solve, by one lane: the camera of scene f beside it (per-scene K) ...
__device__ inline void hypothesis_K(const double *K, int64_t f, double *Kh /* null: one K for all */, int64_t g)
{
    if (!Kh) return;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kh[g * 9 + i] = K[f * 9 + i];
}
// ... and its set: records pick[0 .. 4) of the scene that begins at record beg of scene2 / scene3 (each inside the scene), or, where no
// set could be drawn (!ok: a scene of fewer than four records, a ranking that is none), NaN with idx = -1: the solve then reports a
// non-finite pose.
__device__ inline void write_point_set(bool ok, const int *pick, int64_t beg, const double *scene2, const double *scene3, int64_t g,
                                       int32_t *idx /* optional */, double *p2, double *p3)
{
    if (!ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (idx) idx[g * 4 + j] = -1;
            p2[(g * 4 + j) * 2] = NAN; p2[(g * 4 + j) * 2 + 1] = NAN;
            p3[(g * 4 + j) * 3] = NAN; p3[(g * 4 + j) * 3 + 1] = NAN; p3[(g * 4 + j) * 3 + 2] = NAN;
        }
        return;
    }
    const double *s2 = scene2 + beg * 2, *s3 = scene3 + beg * 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = pick[j];
        if (idx) idx[g * 4 + j] = c;
        p2[(g * 4 + j) * 2] = s2[c * 2]; p2[(g * 4 + j) * 2 + 1] = s2[c * 2 + 1];
        p3[(g * 4 + j) * 3] = s3[c * 3]; p3[(g * 4 + j) * 3 + 1] = s3[c * 3 + 1]; p3[(g * 4 + j) * 3 + 2] = s3[c * 3 + 2];
    }
}
// the uniform set of hypothesis h (index within the scene: the Philox counter) of the scene sl
__device__ inline void uniform_hypothesis(Slice sl, uint64_t seed, int32_t h, const double *scene2, const double *scene3, int64_t g, int32_t *idx, double *p2,
                                          double *p3)
{
    int pick[4];
    if (sl.n < 4) return write_point_set(false, pick, sl.beg, scene2, scene3, g, idx, p2, p3); // (refused by the Python entry point: no draw is possible)
    draw_minimal_set(sl.n, seed, (uint32_t)h, pick); // 0 .. M_f - 1 by construction
    write_point_set(true, pick, sl.beg, scene2, scene3, g, idx, p2, p3);
}

} // namespace cvxn
