// devsim_body.h -- TEST-ONLY probe kernels over the DEVICE side of cvxpnpl_amd/csrc/solver_core.h (the
// `#if defined(__HIP_DEVICE_COMPILE__)` branches and whatever hipcc's device pass makes of the rest: FMA contraction).
// Included once by each of the two translation units (devsim.hip: the solver library's unit; devsim_newton2.hip: lane_kernel.hip's,
// CVX_REFINE_NEWTON2) with DS(name) giving the unit's entry names.  Every entry: one element per lane, 256-thread blocks, a bounds
// check, device pointers in and out, hipGetLastError returned.  No formula is restated here: everything is a call into the headers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "solver_core.h"
#include "problem_io.h"

#define DS_LANE(n)                                                    \
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       \
    if (i >= (long)(n)) return
#define DS_LAUNCH(kern, n, ...)                                                             \
    do {                                                                                    \
        if ((n) > 0) hipLaunchKernelGGL(kern, dim3(((n) + 255) / 256), dim3(256), 0, 0, __VA_ARGS__); \
        return (int)hipGetLastError();                                                      \
    } while (0)

namespace {

// ---- scalar maps: 0 rcp, 1 rsqrt_, 2 sqrt_fast
template <int OP>
__global__ void k_scalar(const double *x, double *y, int n)
{
    DS_LANE(n);
    y[i] = OP == 0 ? cvx::rcp(x[i]) : (OP == 1 ? cvx::rsqrt_(x[i]) : cvx::sqrt_fast(x[i]));
}

// ---- rotations (al, be, gam, rot) -> (c, s, t | dl): 0 jacobi_cs(double), 1 jacobi_cs_dl(exact = false), 2 jacobi_cs_dl(exact = true)
template <int OP>
__global__ void k_rot_f64(const double *abg, const int *rot, double *out, int n)
{
    DS_LANE(n);
    double c, s, u;
    if (OP == 0) cvx::jacobi_cs(abg[3 * i], abg[3 * i + 1], abg[3 * i + 2], rot[i] != 0, c, s, u);
    else cvx::jacobi_cs_dl(abg[3 * i], abg[3 * i + 1], abg[3 * i + 2], rot[i] != 0, c, s, u, OP == 2);
    out[3 * i] = c; out[3 * i + 1] = s; out[3 * i + 2] = u;
}
__global__ void k_rot_f32(const float *abg, const int *rot, float *out, int n)
{
    DS_LANE(n);
    float c, s, t;
    cvx::jacobi_cs(abg[3 * i], abg[3 * i + 1], abg[3 * i + 2], rot[i] != 0, c, s, t);
    out[3 * i] = c; out[3 * i + 1] = s; out[3 * i + 2] = t;
}

// ---- eigen test hook of hostsim.cpp (hs_pospart), one matrix per lane: 0 Eig, 1 Eig with exact on, 2 EigF
template <class E>
__device__ __forceinline__ void pospart_lane(bool exact, const double *W, double *Wp, double *lam, int *sweeps)
{
    E e;
    cvx::set_exact(e, exact);
    cvx::eig_load(e, W);
    *sweeps = cvx::eig_solve(e, 30, 1e-30);
    cvx::eig_pospart(e, Wp);
    for (int j = 0; j < 10; ++j) lam[j] = sqrt((double)e.n2[j]) - e.sigma;
}
template <int MODE>
__global__ void k_pospart(const double *W, double *Wp, double *lam, int *sweeps, int n)
{
    DS_LANE(n);
    if (MODE == 2) pospart_lane<cvx::EigF>(false, W + 55 * i, Wp + 55 * i, lam + 10 * i, sweeps + i);
    else pospart_lane<cvx::Eig>(MODE == 1, W + 55 * i, Wp + 55 * i, lam + 10 * i, sweeps + i);
}

__global__ void k_polar3(const double *M, double *R, int iters, int n)
{
    DS_LANE(n);
    double m[9], r[9];
    for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
    cvx::polar3(m, r, iters);
    for (int k = 0; k < 9; ++k) R[9 * i + k] = r[k];
}
__global__ void k_near_rotation(const double *M, double *R, int n)
{
    DS_LANE(n);
    double m[9], r[9];
    for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
    cvx::near_rotation(m, r);
    for (int k = 0; k < 9; ++k) R[9 * i + k] = r[k];
}
__global__ void k_inv3(const double *M, double *Mi, double *det, int n)
{
    DS_LANE(n);
    double m[9], r[9], d;
    for (int k = 0; k < 9; ++k) m[k] = M[9 * i + k];
    cvx::inv3(m, r, d);
    for (int k = 0; k < 9; ++k) Mi[9 * i + k] = r[k];
    det[i] = d;
}

template <int VAR>
__global__ void k_proj_affine(double *E, int homog, int n)
{
    DS_LANE(n);
    double e[55];
    for (int k = 0; k < 55; ++k) e[k] = E[55 * i + k];
    cvx::proj_affine<VAR>(e, homog != 0);
    for (int k = 0; k < 55; ++k) E[55 * i + k] = e[k];
}

__global__ void k_dual_lambda(const double *R, const double *rhs, int symm, double *lam, int n)
{
    DS_LANE(n);
    double r[9], h[10], l[10];
    for (int k = 0; k < 9; ++k) r[k] = R[9 * i + k];
    for (int k = 0; k < 10; ++k) h[k] = rhs[10 * i + k];
    cvx::dual_lambda(r, h, symm != 0, l);
    for (int k = 0; k < 10; ++k) lam[10 * i + k] = l[k];
}

__global__ void k_rounds_to(const double *v, const double *Rp, double tol, int *ok, double *d0, int n)
{
    DS_LANE(n);
    double a[10], r[9], d;
    for (int k = 0; k < 10; ++k) a[k] = v[10 * i + k];
    for (int k = 0; k < 9; ++k) r[k] = Rp[9 * i + k];
    ok[i] = cvx::rounds_to(a, r, d, tol) ? 1 : 0;
    d0[i] = d;
}

__global__ void k_assemble(int n_p, const double *pts_2d, const double *pts_3d, int n_l, const double *line_2d, const double *line_3d,
                           const double *K, int K_per_problem, double *B, double *Q9, int *rc, int n)
{
    DS_LANE(n);
    const cvx::ProblemView pv = cvx::make_view(i, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem);
    double b[27], q[45];
    rc[i] = cvx::assemble(pv, b, q) ? 0 : -1;
    for (int k = 0; k < 27; ++k) B[27 * i + k] = b[k];
    for (int k = 0; k < 45; ++k) Q9[45 * i + k] = q[k];
}

} // namespace

extern "C" {

int DS(scalar)(int op, const double *x, double *y, int n)
{
    if (op == 0) DS_LAUNCH(k_scalar<0>, n, x, y, n);
    if (op == 1) DS_LAUNCH(k_scalar<1>, n, x, y, n);
    if (op == 2) DS_LAUNCH(k_scalar<2>, n, x, y, n);
    return -1;
}
int DS(rot_f64)(int op, const double *abg, const int *rot, double *out, int n)
{
    if (op == 0) DS_LAUNCH(k_rot_f64<0>, n, abg, rot, out, n);
    if (op == 1) DS_LAUNCH(k_rot_f64<1>, n, abg, rot, out, n);
    if (op == 2) DS_LAUNCH(k_rot_f64<2>, n, abg, rot, out, n);
    return -1;
}
int DS(rot_f32)(const float *abg, const int *rot, float *out, int n) { DS_LAUNCH(k_rot_f32, n, abg, rot, out, n); }
int DS(pospart)(int mode, const double *W, double *Wp, double *lam, int *sweeps, int n)
{
    if (mode == 0) DS_LAUNCH(k_pospart<0>, n, W, Wp, lam, sweeps, n);
    if (mode == 1) DS_LAUNCH(k_pospart<1>, n, W, Wp, lam, sweeps, n);
    if (mode == 2) DS_LAUNCH(k_pospart<2>, n, W, Wp, lam, sweeps, n);
    return -1;
}
int DS(polar3)(const double *M, double *R, int iters, int n) { DS_LAUNCH(k_polar3, n, M, R, iters, n); }
int DS(near_rotation)(const double *M, double *R, int n) { DS_LAUNCH(k_near_rotation, n, M, R, n); }
int DS(inv3)(const double *M, double *Mi, double *det, int n) { DS_LAUNCH(k_inv3, n, M, Mi, det, n); }
int DS(proj_affine)(double *E, int homog, int variant, int n)
{
    if (variant == cvx::VAR_RC) DS_LAUNCH(k_proj_affine<cvx::VAR_RC>, n, E, homog, n);
    DS_LAUNCH(k_proj_affine<cvx::VAR_FULL>, n, E, homog, n);
}
int DS(dual_lambda)(const double *R, const double *rhs, int symm, double *lam, int n) { DS_LAUNCH(k_dual_lambda, n, R, rhs, symm, lam, n); }
int DS(rounds_to)(const double *v, const double *Rp, double tol, int *ok, double *d0, int n) { DS_LAUNCH(k_rounds_to, n, v, Rp, tol, ok, d0, n); }
int DS(assemble)(int n_p, const double *pts_2d, const double *pts_3d, int n_l, const double *line_2d, const double *line_3d, const double *K,
                 int K_per_problem, double *B, double *Q9, int *rc, int n)
{
    DS_LAUNCH(k_assemble, n, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, B, Q9, rc, n);
}

} // extern "C"
