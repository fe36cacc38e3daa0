// vjp_core.h -- the backward pass of a certified pose: implicit-function VJP, host and device from one source.
//
// A certified pose (R, t) is the global minimiser over O(3) x R^3 of the reference's algebraic cost (cvxpnpl.py:541-549 with the
// rows reordered):  f = sum_points |[p]x (R X + t)|^2 + sum_line_end_points (n . (R L + t))^2.  Its first-order condition g = 0
// holds there, so the implicit function theorem gives the vector-Jacobian product through one 6x6 solve per problem; nothing of the
// Douglas-Rachford iteration, the SDP or the eigen-extraction is differentiated (DESIGN.md section 11 has the derivation).
//
// Chart.  The pose is perturbed about a point c of the scene (the centre the forward's Gram sums use, cvx::shift_centre):
//   X  ->  exp([w]x) R (X - c) + tc + tau,   tc = R c + t,   xi = (w, tau).
// Any chart gives the same gradients at a stationary point; this one keeps H well conditioned when the world origin is far from the
// scene (the rotation-translation coupling of the plain chart t + tau grows like |c|^2).  With yc = R (X - c), z = yc + tc and the
// per-record 3x3 form T (points: [p]x^T [p]x = |p|^2 I - p p^T; line end points: n n^T), s = T z:
//   f = sum z^T T z,   g = 2 sum (yc x s, s),   H = 2 sum E^T T E + [sum_ww (s yc^T + yc s^T - 2 (s . yc) I)],   E = [-[yc]x, I],
// the bracket being the second-order term of the exponential (it vanishes only for noise-free data: a Gauss-Newton H is wrong).
// Upstream: dL = <G_R, [w]x R> + <g_t, dt> with dt = tau + (R c) x w, so b = (b_w + g_t x (R c), g_t), b_w the axial part of
// G_R R^T.  v = H^-1 b; then dL/dtheta_i = -2 d/dtheta_i [ z_i^T T_i w_i ],  w_i = v_w x yc_i + v_tau  (R, t, v held fixed).
#pragma once
#include <math.h>

#include "problem_io.h"

namespace cvxv {

enum VjpStatus : int { VJP_OK = 0, VJP_SKIPPED = 1, VJP_SINGULAR = 2, VJP_NONFINITE = 3 };

constexpr int ACC_N = 38;     // doubles reduced per problem
constexpr double PIVOT_TOL = 1e-11; // Cholesky pivot below this fraction of its diagonal entry: H is taken as singular

// the sums one problem reduces: H_gn = 2 sum E^T T E (upper triangle, row by row), S = sum s yc^T (row-major), g, f, scale = sum tr(T) |z|^2
struct Acc {
    double v[ACC_N]; // [0,21) H_gn, [21,30) S, [30,36) g, [36] f, [37] scale
};

CVX_HD void acc_zero(Acc &a)
{
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) a.v[i] = 0.0;
}

CVX_HD constexpr int hidx(int i, int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

CVX_HD void cross(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

CVX_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

CVX_HD void sym_mul(const double *T6, const double *x, double *y) // T packed 00 01 02 11 12 22
{
    y[0] = T6[0] * x[0] + T6[1] * x[1] + T6[2] * x[2];
    y[1] = T6[1] * x[0] + T6[3] * x[1] + T6[4] * x[2];
    y[2] = T6[2] * x[0] + T6[4] * x[1] + T6[5] * x[2];
}

// the per-problem constants: K^-1, the chart centre c and tc = R c + t
struct Frame {
    double Ki[9], R[9], c[3], tc[3];
};

CVX_HD bool frame_make(const cvx::ProblemView &pv, const double *R, const double *t, Frame &fr)
{
    double Kc[9], det;
    CVX_UNROLL for (int i = 0; i < 9; ++i) { Kc[i] = pv.K[i]; fr.R[i] = R[i]; }
    cvx::inv3(Kc, fr.Ki, det);
    cvx::shift_centre(pv.n_p, pv.p3, pv.n_l, pv.l3, fr.c);
    CVX_UNROLL for (int i = 0; i < 3; ++i) fr.tc[i] = R[3 * i] * fr.c[0] + R[3 * i + 1] * fr.c[1] + R[3 * i + 2] * fr.c[2] + t[i];
    return det == det && det != 0.0;
}

CVX_HD void point_form(const double *Ki, double u, double v, double *p, double *T6)
{
    cvx::bearing(Ki, u, v, p);
    const double n2 = dot3(p, p);
    T6[0] = n2 - p[0] * p[0]; T6[1] = -p[0] * p[1]; T6[2] = -p[0] * p[2];
    T6[3] = n2 - p[1] * p[1]; T6[4] = -p[1] * p[2]; T6[5] = n2 - p[2] * p[2];
}

// n = (a x b) / |a x b| of a 2D line (u0 v0 u1 v1); also returns a, b and 1 / |a x b| for the backward
CVX_HD void line_form(const double *Ki, const double *l2, double *a, double *b, double *n, double &inv, double *T6)
{
    cvx::bearing(Ki, l2[0], l2[1], a);
    cvx::bearing(Ki, l2[2], l2[3], b);
    cross(a, b, n);
    inv = 1.0 / sqrt(dot3(n, n));
    n[0] *= inv; n[1] *= inv; n[2] *= inv;
    T6[0] = n[0] * n[0]; T6[1] = n[0] * n[1]; T6[2] = n[0] * n[2];
    T6[3] = n[1] * n[1]; T6[4] = n[1] * n[2]; T6[5] = n[2] * n[2];
}

CVX_HD void centred(const Frame &fr, const double *X, double *yc, double *z)
{
    const double d[3] = {X[0] - fr.c[0], X[1] - fr.c[1], X[2] - fr.c[2]};
    CVX_UNROLL for (int i = 0; i < 3; ++i) {
        yc[i] = fr.R[3 * i] * d[0] + fr.R[3 * i + 1] * d[1] + fr.R[3 * i + 2] * d[2];
        z[i] = yc[i] + fr.tc[i];
    }
}

// one record (a point, or one end point of a line) with its form T
CVX_HD void acc_record(Acc &a, const Frame &fr, const double *T6, const double *X)
{
    double yc[3], z[3], s[3], ys[3];
    centred(fr, X, yc, z);
    sym_mul(T6, z, s);
    cross(yc, s, ys);
    // E = [-[yc]x, I] (3 x 6): column k < 3 is e_k x yc
    double E[3][6];
    E[0][0] = 0.0;    E[0][1] = yc[2];  E[0][2] = -yc[1];
    E[1][0] = -yc[2]; E[1][1] = 0.0;    E[1][2] = yc[0];
    E[2][0] = yc[1];  E[2][1] = -yc[0]; E[2][2] = 0.0;
    CVX_UNROLL for (int i = 0; i < 3; ++i) CVX_UNROLL for (int k = 0; k < 3; ++k) E[i][3 + k] = (i == k) ? 1.0 : 0.0;
    double TE[3][6];
    CVX_UNROLL for (int k = 0; k < 6; ++k) {
        const double col[3] = {E[0][k], E[1][k], E[2][k]};
        double o[3];
        sym_mul(T6, col, o);
        TE[0][k] = o[0]; TE[1][k] = o[1]; TE[2][k] = o[2];
    }
    CVX_UNROLL for (int i = 0; i < 6; ++i)
        CVX_UNROLL for (int j = i; j < 6; ++j)
            a.v[hidx(i, j)] += 2.0 * (E[0][i] * TE[0][j] + E[1][i] * TE[1][j] + E[2][i] * TE[2][j]);
    CVX_UNROLL for (int i = 0; i < 3; ++i) CVX_UNROLL for (int j = 0; j < 3; ++j) a.v[21 + 3 * i + j] += s[i] * yc[j];
    CVX_UNROLL for (int i = 0; i < 3; ++i) { a.v[30 + i] += 2.0 * ys[i]; a.v[33 + i] += 2.0 * s[i]; }
    a.v[36] += dot3(z, s);
    a.v[37] += (T6[0] + T6[3] + T6[5]) * dot3(z, z);
}

CVX_HD void acc_point(Acc &a, const Frame &fr, const double *uv, const double *X)
{
    double p[3], T6[6];
    point_form(fr.Ki, uv[0], uv[1], p, T6);
    acc_record(a, fr, T6, X);
}

CVX_HD void acc_line(Acc &a, const Frame &fr, const double *l2, const double *L)
{
    double pa[3], pb[3], n[3], inv, T6[6];
    line_form(fr.Ki, l2, pa, pb, n, inv, T6);
    acc_record(a, fr, T6, L);
    acc_record(a, fr, T6, L + 3);
}

// symmetric 6x6 eigenvalue range by cyclic Jacobi (diagnostics only: vjp_info)
CVX_HD void eig_range6(const double *H, double &lo, double &hi)
{
    double A[6][6];
    CVX_UNROLL for (int i = 0; i < 6; ++i) CVX_UNROLL for (int j = 0; j < 6; ++j) A[i][j] = H[i * 6 + j];
    for (int sweep = 0; sweep < 10; ++sweep) {
        double off = 0.0, dia = 0.0;
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int j = 0; j < 6; ++j) {
                if (i != j) off += A[i][j] * A[i][j];
                else dia += A[i][j] * A[i][j];
            }
        if (!(off > 1e-30 * dia)) break;
        CVX_UNROLL for (int p = 0; p < 5; ++p)
            CVX_UNROLL for (int q = p + 1; q < 6; ++q) {
                if (A[p][q] == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                CVX_UNROLL for (int k = 0; k < 6; ++k) { // A <- J^T A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = cs * akp - sn * akq;
                    A[k][q] = sn * akp + cs * akq;
                }
                CVX_UNROLL for (int k = 0; k < 6; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = cs * apk - sn * aqk;
                    A[q][k] = sn * apk + cs * aqk;
                }
            }
    }
    lo = hi = A[0][0];
    CVX_UNROLL for (int i = 1; i < 6; ++i) { lo = A[i][i] < lo ? A[i][i] : lo; hi = A[i][i] > hi ? A[i][i] : hi; }
}

// From the reduced sums to v = H^-1 b (returned in v[6]; zeros unless VJP_OK).  gR [9] / gt [3] may be NULL (zero).
// info [2] (filled when want_info): lambda_min(H) / lambda_max(H), and |g| / (2 sqrt(tr(H_gn) (f + 1e-20 scale))), which is <= 1 by
// Cauchy-Schwarz and 0 at an exactly stationary pose.
// ncorr = points + lines.  Each gives two equations, so fewer than three determine no pose: VJP_SINGULAR whatever H looks like.  (At a
// stationary pose the pivot test finds that by itself; away from one the second-order term lifts the null space of H_gn by about the
// relative residual, far above PIVOT_TOL, and a meaningless v would pass for VJP_OK.)
CVX_HD int solve_v(const Acc &a, const Frame &fr, int ncorr, const double *gR, const double *gt, double *v, double *info, bool want_info)
{
    CVX_UNROLL for (int i = 0; i < 6; ++i) v[i] = 0.0;
    double H[36];
    CVX_UNROLL for (int i = 0; i < 6; ++i) CVX_UNROLL for (int j = 0; j < 6; ++j) H[i * 6 + j] = a.v[hidx(i, j)];
    const double trS = a.v[21] + a.v[25] + a.v[29];
    CVX_UNROLL for (int i = 0; i < 3; ++i)
        CVX_UNROLL for (int j = 0; j < 3; ++j) H[i * 6 + j] += a.v[21 + 3 * i + j] + a.v[21 + 3 * j + i] - (i == j ? 2.0 * trS : 0.0);
    double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g_t[3] = {0, 0, 0};
    if (gR) CVX_UNROLL for (int i = 0; i < 9; ++i) G[i] = gR[i];
    if (gt) CVX_UNROLL for (int i = 0; i < 3; ++i) g_t[i] = gt[i];
    double M[9]; // G_R R^T
    CVX_UNROLL for (int i = 0; i < 3; ++i)
        CVX_UNROLL for (int j = 0; j < 3; ++j) M[3 * i + j] = G[3 * i] * fr.R[3 * j] + G[3 * i + 1] * fr.R[3 * j + 1] + G[3 * i + 2] * fr.R[3 * j + 2];
    double Rc[3], gRc[3];
    CVX_UNROLL for (int i = 0; i < 3; ++i) Rc[i] = fr.R[3 * i] * fr.c[0] + fr.R[3 * i + 1] * fr.c[1] + fr.R[3 * i + 2] * fr.c[2];
    cross(g_t, Rc, gRc);
    double b[6] = {M[7] - M[5] + gRc[0], M[2] - M[6] + gRc[1], M[3] - M[1] + gRc[2], g_t[0], g_t[1], g_t[2]};
    double gn = 0.0, trH = 0.0;
    CVX_UNROLL for (int i = 0; i < 6; ++i) { gn += a.v[30 + i] * a.v[30 + i]; trH += a.v[hidx(i, i)]; }
    bool finite = true;
    CVX_UNROLL for (int i = 0; i < 36; ++i) finite = finite && (H[i] - H[i] == 0.0);
    CVX_UNROLL for (int i = 0; i < 6; ++i) finite = finite && (b[i] - b[i] == 0.0);
    CVX_UNROLL for (int i = 0; i < 12; ++i) finite = finite && ((i < 9 ? fr.R[i] : fr.tc[i - 9]) - (i < 9 ? fr.R[i] : fr.tc[i - 9]) == 0.0);
    info[0] = info[1] = NAN;
    if (want_info) {
        double lo = NAN, hi = NAN;
        if (finite) eig_range6(H, lo, hi);
        info[0] = lo / hi;
        info[1] = sqrt(gn) / (2.0 * sqrt(trH * (a.v[36] + 1e-20 * a.v[37])) + 1e-300);
    }
    if (!finite) return VJP_NONFINITE;
    if (ncorr < 3) return VJP_SINGULAR;
    // Cholesky H = L L^T in place (lower triangle), pivot relative to its own diagonal entry
    double Lm[36];
    CVX_UNROLL for (int i = 0; i < 36; ++i) Lm[i] = H[i];
    CVX_UNROLL for (int j = 0; j < 6; ++j) {
        double d = Lm[j * 6 + j];
        CVX_UNROLL for (int k = 0; k < j; ++k) d -= Lm[j * 6 + k] * Lm[j * 6 + k];
        if (!(d > PIVOT_TOL * H[j * 6 + j])) return VJP_SINGULAR;
        const double r = sqrt(d), ri = 1.0 / r;
        Lm[j * 6 + j] = r;
        CVX_UNROLL for (int i = j + 1; i < 6; ++i) {
            double x = Lm[i * 6 + j];
            CVX_UNROLL for (int k = 0; k < j; ++k) x -= Lm[i * 6 + k] * Lm[j * 6 + k];
            Lm[i * 6 + j] = x * ri;
        }
    }
    double y[6];
    CVX_UNROLL for (int i = 0; i < 6; ++i) {
        double x = b[i];
        CVX_UNROLL for (int k = 0; k < i; ++k) x -= Lm[i * 6 + k] * y[k];
        y[i] = x / Lm[i * 6 + i];
    }
    double x6[6];
    CVX_UNROLL for (int ii = 0; ii < 6; ++ii) {
        const int i = 5 - ii;
        double x = y[i];
        CVX_UNROLL for (int k = i + 1; k < 6; ++k) x -= Lm[k * 6 + i] * x6[k];
        x6[i] = x / Lm[i * 6 + i];
    }
    bool ok = true;
    CVX_UNROLL for (int i = 0; i < 6; ++i) ok = ok && (x6[i] - x6[i] == 0.0);
    if (!ok) return VJP_NONFINITE;
    CVX_UNROLL for (int i = 0; i < 6; ++i) v[i] = x6[i];
    return VJP_OK;
}

// d phi / d X and d phi / d z-side of one record, phi = z^T T w, w = v_w x yc + v_tau:  returns Tz (= s) and Tw, and adds
// d phi / dX = R^T (T w - v_w x s) to gX (scaled by -2 at the caller)
CVX_HD void record_parts(const Frame &fr, const double *v, const double *X, double *z, double *w)
{
    double yc[3], vy[3];
    centred(fr, X, yc, z);
    cross(v, yc, vy);
    CVX_UNROLL for (int i = 0; i < 3; ++i) w[i] = vy[i] + v[3 + i];
}

// -2 d phi / dX = -2 R^T (T w - v_w x T z)
CVX_HD void grad_X(const Frame &fr, const double *v, const double *T6, const double *z, const double *w, double *gX)
{
    double s[3], Tw[3], vs[3], d[3];
    sym_mul(T6, z, s);
    sym_mul(T6, w, Tw);
    cross(v, s, vs);
    CVX_UNROLL for (int i = 0; i < 3; ++i) d[i] = Tw[i] - vs[i];
    CVX_UNROLL for (int j = 0; j < 3; ++j) gX[j] = -2.0 * (fr.R[j] * d[0] + fr.R[3 + j] * d[1] + fr.R[6 + j] * d[2]);
}

// pixel gradient from d phi / d p (p = K^-1 (u, v, 1)): -2 K^-1[:, :2]^T dp
CVX_HD void grad_pixel(const double *Ki, const double *dp, double *g2)
{
    g2[0] = -2.0 * (Ki[0] * dp[0] + Ki[3] * dp[1] + Ki[6] * dp[2]);
    g2[1] = -2.0 * (Ki[1] * dp[0] + Ki[4] * dp[1] + Ki[7] * dp[2]);
}

// VJP of one point correspondence: g2 [2] (pixel), g3 [3] (3D point); either may be NULL
CVX_HD void vjp_point(const Frame &fr, const double *v, const double *uv, const double *X, double *g2, double *g3)
{
    double p[3], T6[6], z[3], w[3];
    point_form(fr.Ki, uv[0], uv[1], p, T6);
    record_parts(fr, v, X, z, w);
    if (g3) grad_X(fr, v, T6, z, w, g3);
    if (g2) {
        // phi = |p|^2 (z.w) - (p.z)(p.w)
        const double zw = dot3(z, w), pz = dot3(p, z), pw = dot3(p, w);
        double dp[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i) dp[i] = 2.0 * p[i] * zw - z[i] * pw - w[i] * pz;
        grad_pixel(fr.Ki, dp, g2);
    }
}

// VJP of one line correspondence: g2 [4] (u0 v0 u1 v1), g3 [6] (both end points); either may be NULL
CVX_HD void vjp_line(const Frame &fr, const double *v, const double *l2, const double *L, double *g2, double *g3)
{
    double pa[3], pb[3], n[3], inv, T6[6], z0[3], w0[3], z1[3], w1[3];
    line_form(fr.Ki, l2, pa, pb, n, inv, T6);
    record_parts(fr, v, L, z0, w0);
    record_parts(fr, v, L + 3, z1, w1);
    if (g3) {
        grad_X(fr, v, T6, z0, w0, g3);
        grad_X(fr, v, T6, z1, w1, g3 + 3);
    }
    if (g2) {
        // phi = sum_k (n.z_k)(n.w_k):  d phi / dn = sum_k z_k (n.w_k) + w_k (n.z_k); through n = m / |m|, m = a x b
        const double nw0 = dot3(n, w0), nz0 = dot3(n, z0), nw1 = dot3(n, w1), nz1 = dot3(n, z1);
        double q[3], gm[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i) q[i] = z0[i] * nw0 + w0[i] * nz0 + z1[i] * nw1 + w1[i] * nz1;
        const double nq = dot3(n, q);
        CVX_UNROLL for (int i = 0; i < 3; ++i) gm[i] = (q[i] - n[i] * nq) * inv;
        double da[3], db[3]; // d (m . gm) / da = b x gm,  / db = gm x a
        cross(pb, gm, da);
        cross(gm, pa, db);
        grad_pixel(fr.Ki, da, g2);
        grad_pixel(fr.Ki, db, g2 + 2);
    }
}

// status s admitted by mask: bit s
CVX_HD bool admitted(int status, uint32_t mask) { return status >= 0 && status < 32 && ((mask >> status) & 1u); }

} // namespace cvxv
