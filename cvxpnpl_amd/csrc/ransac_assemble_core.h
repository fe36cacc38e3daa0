// ransac_assemble_core.h -- the cost (B27, Q45, count) of a chosen SUBSET of a scene's correspondences, ONE statement of it for the four
// kernels that assemble one -- cvxn::assemble_consensus_kernel and cvxnl::assemble_consensus_kernel (chosen by masks, one wavefront per
// scene), cvxnlo::lo_assemble_active_kernel and cvxnllo::lo_assemble_pnpl_active_kernel (chosen by inlier predicates, four wavefronts per
// entry) -- and for the host replica of the last two (assemble_entry; DESIGN.md sections 13, 14, 24, 25):
//   centre    = cvx::shift_centre of the first three chosen 3D records in scene order, points before lines, a line giving its two end
//               points (any centre is exact)                                                                          (centre)
//   a lane    strides over the scene with 60 running sums about that centre                                            (the caller's loop)
//   a wave    adds its 64 lanes' sums in the XOR butterfly o = 1, 2, 4, 8, 16, 32, v <- v + v[lane ^ o]               (wave_butterfly)
//   an entry of four waves adds the wave sums in wave order, ((w0 + w1) + w2) + w3                                    (waves_total)
//   the cost  = cvx::gram_finish of the total, the centre put back into B                                             (finish)
//   NaN       for fewer than three chosen, a singular N^T N or a singular K, with the count reported                  (store_cost)
// so the result depends on the inputs alone, and the device and the host agree bit for bit.  What CHOOSES a correspondence (a mask, a
// predicate) and the lane's loop stay with the caller.  No kernel here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "problem_io.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxas {

constexpr int LANES = cvxn::SCENE_BLOCK;  // lanes of a four-wave assembly: the family's workgroup
constexpr int WAVES = cvxn::SCENE_WAVES;
constexpr int GRAM = 60;                  // doubles of a cvx::Gram
static_assert(sizeof(cvx::Gram) == GRAM * sizeof(double), "a Gram is 60 doubles and nothing else");

// ---- the point centre: cvx::shift_centre of the nf <= 3 first chosen correspondences first[0 .. nf) (scene order); none: the origin
__host__ __device__ inline void centre(int nf, const int *first, const double *s3, double *c)
{
    c[0] = c[1] = c[2] = 0.0;
    if (nf <= 0) return;
    double first3[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { // (entries beyond nf repeat the first record and are not read by shift_centre)
        const int m = k < nf ? first[k] : first[0];
        first3[3 * k] = s3[3 * m]; first3[3 * k + 1] = s3[3 * m + 1]; first3[3 * k + 2] = s3[3 * m + 2];
    }
    cvx::shift_centre(nf, first3, 0, nullptr, c);
}

// ---- how many lines the point-and-line centre reads after nfp <= 3 chosen points: none after three, one after one or two, two after none
__host__ __device__ inline int centre_lines_wanted(int nfp) { return nfp >= 3 ? 0 : (nfp == 0 ? 2 : 1); }

// ---- the point-and-line centre: cvx::shift_centre of the first three chosen records, the nfp <= 3 first chosen points fp[0 .. nfp) and
// then the end points of the nfl <= centre_lines_wanted(nfp) first chosen lines fl[0 .. nfl) (scene order); nothing chosen: the origin.
// The centre cvxpnpl_assemble_batch uses on the gathered set.
__host__ __device__ inline void centre(int nfp, const int *fp, int nfl, const int *fl, const double *p3, const double *l3, double *c)
{
    c[0] = c[1] = c[2] = 0.0;
    const int nrec = nfp + 2 * nfl < 3 ? nfp + 2 * nfl : 3;
    if (nrec <= 0) return;
    double first3[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { // (entries beyond nrec repeat the first record and are not read by shift_centre)
        const int kk = k < nrec ? k : 0;
        const double *r;
        if (kk < nfp) {
            r = p3 + 3 * (int64_t)(kk == 0 ? fp[0] : (kk == 1 ? fp[1] : fp[2]));
        } else {
            const int e = kk - nfp; // end point e of the chosen lines: line e / 2, end e % 2
            r = l3 + 6 * (int64_t)(e < 2 ? fl[0] : fl[1]) + 3 * (e & 1);
        }
        first3[3 * k] = r[0]; first3[3 * k + 1] = r[1]; first3[3 * k + 2] = r[2];
    }
    cvx::shift_centre(nrec, first3, 0, nullptr, c);
}

// ---- sum e of an entry from the WAVES wave sums part[w * stride + e], in wave order
__host__ __device__ inline double waves_total(const double *part, int stride, int e)
{
    double tot = part[e];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) tot += part[w * stride + e];
    return tot;
}

// ---- B27 and Q45 from the total sums of n chosen correspondences: cvx::gram_finish, the centre put back into B.  Returns whether the
// cost is usable: at least three chosen, N^T N regular, K (determinant det) regular.
__host__ __device__ inline bool finish(const cvx::Gram &g, int n, double det, const double *c, double *B, double *Q9)
{
    const bool ok = n >= 3 && cvx::gram_finish(g, B, Q9) && (det == det) && det != 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j];
    return ok;
}

// ---- row `row` of the outputs, by ONE lane: the cost, or NaN where it is not usable; the count either way.  (Static indices keep B and
// Q9 in registers.)
__host__ __device__ inline void store_cost(bool ok, const double *B, const double *Q9, int n, int64_t row, double *B27, double *Q45, int32_t *count)
{
#pragma unroll
    for (int i = 0; i < 27; ++i) B27[row * 27 + i] = ok ? B[i] : NAN;
#pragma unroll
    for (int i = 0; i < 45; ++i) Q45[row * 45 + i] = ok ? Q9[i] : NAN;
    count[row] = n;
}

// ---- the host replica of a four-wave assembly, serially: lane l's sums and count from lane_sums(l, g), the butterfly of each wave by
// index l ^ o, the four wave sums (lane 0 of each wave) in wave order, the finish and the store of row `row`
template <class LaneSums>
inline void assemble_entry(int64_t row, const double *c, double det, LaneSums lane_sums, double *B27, double *Q45, int32_t *count)
{
    std::vector<double> v(LANES * GRAM), nv(LANES * GRAM);
    int n = 0;
    for (int l = 0; l < LANES; ++l) n += lane_sums(l, *reinterpret_cast<cvx::Gram *>(&v[l * GRAM]));
    for (int o = 1; o < 64; o <<= 1) { // v <- v + v[lane ^ o], within each wave
        for (int l = 0; l < LANES; ++l)
            for (int e = 0; e < GRAM; ++e) nv[l * GRAM + e] = v[l * GRAM + e] + v[(l ^ o) * GRAM + e];
        v.swap(nv);
    }
    cvx::Gram total;
    for (int e = 0; e < GRAM; ++e) reinterpret_cast<double *>(&total)[e] = waves_total(v.data(), 64 * GRAM, e);
    double B[27], Q9[45];
    const bool ok = finish(total, n, det, c, B, Q9);
    store_cost(ok, B, Q9, n, row, B27, Q45, count);
}

// ---- the device side

// a value every lane of the wavefront holds, moved to the scalar registers: the camera, K^-1 and the centre of a four-wave assembly are
// workgroup-uniform and read in every iteration of its loops, beside 60 running sums per lane
__device__ inline double wave_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int N>
__device__ inline void wave_uniform(double (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_uniform(v[i]);
}

__device__ inline double wave_xor_add(double v, int o) { return v + __shfl_xor(v, o); }

// the butterfly: afterwards every lane of the wavefront holds the wave's 60 sums and its count
__device__ inline void wave_butterfly(cvx::Gram &g, int &n)
{
#pragma unroll 1
    for (int o = 1; o < 64; o <<= 1) { // (rolled: six passes over the same 60 sums; in groups of twelve, so that the exchanged values of
                                       // a pass are never all in flight beside the sums)
#pragma unroll
        for (int i = 0; i < 6; ++i) g.M0[i] = wave_xor_add(g.M0[i], o);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int i = 0; i < 6; ++i) g.M1[k][i] = wave_xor_add(g.M1[k][i], o);
            if (k != 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int i = 0; i < 6; ++i) g.M2[k][i] = wave_xor_add(g.M2[k][i], o);
            if (k & 1) __builtin_amdgcn_sched_barrier(0);
        }
        n += __shfl_xor(n, o);
    }
}

// the 60 sums of a Gram to a flat array, by static indices (registers)
__device__ inline void gram_store(const cvx::Gram &g, double *dst)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) dst[i] = g.M0[i];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[6 + k * 6 + i] = g.M1[k][i];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[24 + k * 6 + i] = g.M2[k][i];
}

// positions of the first `want` (at most 3) of n correspondences that pass pred(m), in scene order, by ONE wavefront: ballots over chunks
// of 64 (wave-uniform)
template <class Pred>
__device__ inline int wave_first(int n, int want, int *first, Pred pred)
{
    const int lane = threadIdx.x;
    int nf = 0;
    for (int64_t base = 0; base < n && nf < want; base += 64) {
        const int64_t m = base + lane;
        unsigned long long b = __ballot(m < n && pred(m));
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

// the tail of a four-wave assembly, called by every lane of the workgroup after its wave's butterfly (barriers): the four wave sums and
// counts meet in LDS in wave order, and wavefront 0 finishes from the totals in LDS -- so that the sums of the loops and B, Q of the
// finish are never live together -- and stores row `row`
__device__ inline void block_finish_store(const cvx::Gram &g, int n_wave, double *part /* LDS, WAVES * GRAM */, double *total /* LDS, GRAM */,
                                          int *cnt_w /* LDS, WAVES */, double det, const double *c, int64_t row, double *B27, double *Q45, int32_t *count)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) { // (every lane of the wave holds the wave's sums)
        gram_store(g, part + wave * GRAM);
        cnt_w[wave] = n_wave;
    }
    __syncthreads();
    if (tid < GRAM) total[tid] = waves_total(part, GRAM, tid);
    int n = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) n += cnt_w[w];
    __syncthreads();
    if (wave != 0) return; // (no barrier below)
    double B[27], Q9[45];
    const bool ok = finish(*reinterpret_cast<const cvx::Gram *>(total), n, det, c, B, Q9);
    if (tid == 0) store_cost(ok, B, Q9, n, row, B27, Q45, count); // (every lane holds the same values)
}

} // namespace cvxas
