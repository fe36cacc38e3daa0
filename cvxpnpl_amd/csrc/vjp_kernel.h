// vjp_kernel.h -- the pose VJP on the device (cvxpnpl_pose_vjp_batch); the mathematics is vjp_core.h, shared with the host path.
//
// Per problem: a reduction of 38 sums over the correspondences, a 6x6 Cholesky solve, then a scatter that writes every
// correspondence's gradient.  Two regimes, as in the forward:
//   small N  vjp_group_kernel: 16 lanes per problem, four problems per wavefront (the quad layout).  Lane l takes correspondences
//            l, l + 16, ...; the sums meet across the 16 lanes by xor exchanges (ds_bpermute), every lane solves the 6x6 itself and
//            writes its own correspondences' gradients.  One launch, no LDS.
//   large N  (records >= VJP_LARGE_N) few problems with many correspondences: vjp_reduce_kernel (nblk workgroups per problem stream the
//            records, partial sums in scratch), vjp_solve_kernel (one lane per problem adds the partials in a fixed order and solves),
//            vjp_scatter_kernel (one lane per correspondence).  Deterministic.
#pragma once
#include "vjp_core.h"

namespace cvxv {

constexpr int VJP_LARGE_N = 768; // records (points + 2 lines) from which the multi-block path runs (the forward's LARGE_N)
constexpr int VJP_TPB = 256;
constexpr int VJP_STRIDE = 16;   // doubles per problem of the solve kernel's output: v [6], ok flag, c [3], tc [3]

struct VjpArgs {
    int64_t batch;
    int n_p, n_l, K_per_problem;
    uint32_t admit;
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *gR, *gt;
    const int32_t *status;
    double *g2, *g3, *gl2, *gl3, *info;
    int32_t *vstatus;
};

__device__ __forceinline__ cvx::ProblemView vjp_view(const VjpArgs &a, int64_t b)
{
    return cvx::make_view(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem);
}

__device__ __forceinline__ void vjp_corr(const VjpArgs &a, const cvx::ProblemView &pv, const Frame &fr, const double *v, int64_t b, int k, bool zero)
{
    if (k < a.n_p) {
        const int64_t i = b * a.n_p + k;
        double g2[2] = {0.0, 0.0}, g3[3] = {0.0, 0.0, 0.0};
        if (!zero) vjp_point(fr, v, pv.p2 + 2 * k, pv.p3 + 3 * k, g2, g3); // (both always: a selected pointer would put the arrays in scratch)
        if (a.g2) { a.g2[2 * i] = g2[0]; a.g2[2 * i + 1] = g2[1]; }
        if (a.g3) CVX_UNROLL for (int j = 0; j < 3; ++j) a.g3[3 * i + j] = g3[j];
    } else {
        const int kl = k - a.n_p;
        const int64_t i = b * a.n_l + kl;
        double g2[4] = {0.0, 0.0, 0.0, 0.0}, g3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (!zero) vjp_line(fr, v, pv.l2 + 4 * kl, pv.l3 + 6 * kl, g2, g3);
        if (a.gl2) CVX_UNROLL for (int j = 0; j < 4; ++j) a.gl2[4 * i + j] = g2[j];
        if (a.gl3) CVX_UNROLL for (int j = 0; j < 6; ++j) a.gl3[6 * i + j] = g3[j];
    }
}

__device__ __forceinline__ void acc_corr(Acc &acc, const cvx::ProblemView &pv, const Frame &fr, int n_p, int k)
{
    if (k < n_p) acc_point(acc, fr, pv.p2 + 2 * k, pv.p3 + 3 * k);
    else acc_line(acc, fr, pv.l2 + 4 * (k - n_p), pv.l3 + 6 * (k - n_p));
}

// ---- small N: 16 lanes per problem ----
template <bool INFO>
__global__ void __launch_bounds__(VJP_TPB) vjp_group_kernel(VjpArgs a)
{
    const int lane = threadIdx.x & 15;
    const int64_t b = (int64_t)blockIdx.x * (VJP_TPB / 16) + (threadIdx.x >> 4);
    if (b >= a.batch) return; // whole groups: the xor exchanges below stay inside a group
    const int ncorr = a.n_p + a.n_l;
    const bool adm = !a.status || admitted(a.status[b], a.admit);
    const cvx::ProblemView pv = vjp_view(a, b);
    Frame fr;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int st = VJP_SKIPPED;
    if (adm) {
        frame_make(pv, a.R + 9 * b, a.t + 3 * b, fr);
        Acc acc;
        acc_zero(acc);
        for (int k = lane; k < ncorr; k += 16) acc_corr(acc, pv, fr, a.n_p, k);
        CVX_UNROLL for (int i = 0; i < ACC_N; ++i) {
            double x = acc.v[i];
            x += __shfl_xor(x, 8, 16);
            x += __shfl_xor(x, 4, 16);
            x += __shfl_xor(x, 2, 16);
            x += __shfl_xor(x, 1, 16);
            acc.v[i] = x;
        }
        double info[2];
        st = solve_v(acc, fr, a.n_p + a.n_l, a.gR ? a.gR + 9 * b : nullptr, a.gt ? a.gt + 3 * b : nullptr, v, info, INFO);
        if (INFO && lane == 0) { a.info[2 * b] = info[0]; a.info[2 * b + 1] = info[1]; }
    } else if (INFO && lane == 0) {
        a.info[2 * b] = NAN; a.info[2 * b + 1] = NAN;
    }
    if (lane == 0) a.vstatus[b] = st;
    for (int k = lane; k < ncorr; k += 16) vjp_corr(a, pv, fr, v, b, k, st != VJP_OK);
}

// ---- large N: partial sums, solve, scatter ----
__host__ __device__ inline int vjp_blocks(int64_t ncorr, int64_t batch)
{
    int64_t want = (2048 + batch - 1) / (batch > 0 ? batch : 1); // fill the chip ...
    const int64_t cap = (ncorr + 4 * VJP_TPB - 1) / (4 * VJP_TPB); // ... with at least 4 correspondences per lane
    want = want > cap ? cap : want;
    return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}

__global__ void __launch_bounds__(VJP_TPB) vjp_reduce_kernel(VjpArgs a, int nblk, double *partial)
{
    __shared__ double red[VJP_TPB / 64][ACC_N];
    const int64_t b = blockIdx.y;
    if (a.status && !admitted(a.status[b], a.admit)) return; // (uniform over the workgroup)
    const int ncorr = a.n_p + a.n_l;
    const cvx::ProblemView pv = vjp_view(a, b);
    Frame fr;
    frame_make(pv, a.R + 9 * b, a.t + 3 * b, fr);
    Acc acc;
    acc_zero(acc);
    for (int k = blockIdx.x * VJP_TPB + threadIdx.x; k < ncorr; k += nblk * VJP_TPB) acc_corr(acc, pv, fr, a.n_p, k);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) {
        double x = acc.v[i];
        CVX_UNROLL for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        if (lane == 0) red[wave][i] = x;
    }
    __syncthreads();
    if (threadIdx.x < ACC_N) {
        double x = red[0][threadIdx.x];
        CVX_UNROLL for (int w = 1; w < VJP_TPB / 64; ++w) x += red[w][threadIdx.x];
        partial[((int64_t)b * nblk + blockIdx.x) * ACC_N + threadIdx.x] = x;
    }
}

__global__ void __launch_bounds__(64) vjp_solve_kernel(VjpArgs a, int nblk, const double *partial, double *vs)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.batch) return;
    double *o = vs + b * VJP_STRIDE;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int st = VJP_SKIPPED;
    Frame fr;
    const cvx::ProblemView pv = vjp_view(a, b);
    frame_make(pv, a.R + 9 * b, a.t + 3 * b, fr);
    double info[2] = {NAN, NAN};
    if (!a.status || admitted(a.status[b], a.admit)) {
        Acc acc;
        acc_zero(acc);
        for (int k = 0; k < nblk; ++k) {
            const double *p = partial + ((int64_t)b * nblk + k) * ACC_N;
            CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc.v[i] += p[i];
        }
        st = solve_v(acc, fr, a.n_p + a.n_l, a.gR ? a.gR + 9 * b : nullptr, a.gt ? a.gt + 3 * b : nullptr, v, info, a.info != nullptr);
    }
    if (a.info) { a.info[2 * b] = info[0]; a.info[2 * b + 1] = info[1]; }
    a.vstatus[b] = st;
    for (int i = 0; i < 6; ++i) o[i] = v[i];
    o[6] = st == VJP_OK ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) { o[7 + i] = fr.c[i]; o[10 + i] = fr.tc[i]; }
}

__global__ void __launch_bounds__(VJP_TPB) vjp_scatter_kernel(VjpArgs a, const double *vs)
{
    const int ncorr = a.n_p + a.n_l;
    const int64_t i = (int64_t)blockIdx.x * VJP_TPB + threadIdx.x;
    if (i >= a.batch * ncorr) return;
    const int64_t b = i / ncorr;
    const int k = (int)(i - b * ncorr);
    const double *o = vs + b * VJP_STRIDE;
    const cvx::ProblemView pv = vjp_view(a, b);
    Frame fr;
    double Kc[9], det;
    for (int j = 0; j < 9; ++j) { Kc[j] = pv.K[j]; fr.R[j] = a.R[9 * b + j]; }
    cvx::inv3(Kc, fr.Ki, det);
    double v[6];
    for (int j = 0; j < 6; ++j) v[j] = o[j];
    for (int j = 0; j < 3; ++j) { fr.c[j] = o[7 + j]; fr.tc[j] = o[10 + j]; }
    vjp_corr(a, pv, fr, v, b, k, o[6] != 1.0);
}

} // namespace cvxv
