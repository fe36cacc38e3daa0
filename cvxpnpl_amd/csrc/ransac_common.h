// ransac_common.h -- what the two RANSAC libraries share (libcvxpnpl_amd_ransac.so: ransac_kernel.h, points; libcvxpnpl_amd_ransac_pnpl.so:
// ransac_pnpl_kernel.h, points and lines): the clamped slice of a scene, the Philox generator of the samplers and the point inlier
// predicate.  ONE definition of each (block_inliers, the mask of one pose by a workgroup of SCENE_BLOCK lanes, among them: the selection and refit
// kernels of ransac_kernel.h and the round update of ransac_adaptive_kernel.h write their masks with it), and no kernel: a library that includes this header compiles nothing it does not launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvxn {

constexpr int SCENE_BLOCK = 256;  // lanes of the sampling / scoring / selection / refit workgroups
constexpr int SCENE_WAVES = SCENE_BLOCK / 64;

struct Slice { int64_t beg; int32_t n; };
__device__ inline Slice scene_slice(const int64_t *off, int64_t f, int64_t n_total)
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

} // namespace cvxn
