// refine_vjp_core.h -- the backward pass of a refined pose: implicit-function VJP of the reprojection minimum, host and device from one
// source.  refine_core.h is included, not edited: records, steps, the projection, the chart, the Cholesky and the
// three lane classes are its own.
//
// A converged refinement is a strict local minimum of f = 1/2 sum rho^2 over the live records' steps (refine_core.h: a step is
// rho = alpha u + beta v + gamma of one projected 3D point).  Its first-order condition g = 0 holds there, so the implicit function
// theorem gives dL/d(correspondences) from one 6x6 solve per problem; nothing of the Levenberg-Marquardt iteration is differentiated.
//
// Chart (that of refine_problem): X -> exp([w]x) R (X - c) + tc + tau, c the mean of the live 3D records, tc = R c + t, y = R (X - c),
// Y = y + tc, h = K Y.  Per step, with K_i the rows of K:
//   q = d rho / dY = (alpha (K_0 - u K_2) + beta (K_1 - v K_2)) / h_2,     J = [y x q, q],     k = [y x K_2, K_2],
//   d q / dY = Q = -(K_2 q^T + q K_2^T) / h_2,  E = [-[y]x, I],  so that  E^T Q E = -(k J^T + J k^T) / h_2,
//   and the second-order term of the exponential map adds  S_ww = 1/2 (q y^T + y q^T) - (q . y) I  to the ww block:
//   H = sum J J^T + rho (E^T Q E + S)       -- the FULL Hessian.  The Gauss-Newton matrix of the forward loop is not enough: at 1 px of
//   noise its gradients are off by 1e-3 relative.
// Upstream: dL = <G_R, [w]x R> + <g_t, tau_pub> with tau_pub = tau + (R c) x w, so b = (b_w + g_t x (R c), g_t), b_w the axial vector of
// G_R R^T - R G_R^T.  psi = H^-1 b = (a, b'); then with e = a x y + b' and s = q . e,  dL/dtheta = -d/dtheta sum rho s  (pose and psi held
// fixed; c too: any chart gives the same gradients at a stationary point).
#pragma once
#include "refine_core.h"

namespace cvxrg {

using cvxr::Pose;
using cvxr::Prob;
using cvxr::Rec;

enum RefineVjpStatus : int { RVJP_OK = 0, RVJP_SKIPPED = 1, RVJP_SINGULAR = 2, RVJP_BEHIND = 3 };

constexpr int ACC_N = cvxr::ACC_N; // [0,21) H (upper triangle, row by row), [21,27) g = sum J rho, [27] sum |J| |rho| (infinite when a live record has depth <= 0)

// where one problem's gradients go: [n_p][2], [n_p][3], [n_l][2][2], [n_l][2][3]; any may be null (not wanted)
struct Grads {
    double *p2, *p3, *l2, *l3;
};

CVX_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the sums of one record at the pose (nothing for a record that is not live)
CVX_HD void rec_acc_full(const Rec &r, const Pose &ps, double *a)
{
    if (r.kind == 0) return;
    CVX_ROLLED for (int s = 0; s < 2; ++s) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        cvxr::rec_step(r, s, X, alpha, beta, gamma);
        const bool front = cvxr::project(ps, X, yc, u, v, iw);
        double j[6], k[6], q[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            q[i] = (alpha * (ps.K[i] - u * ps.K[6 + i]) + beta * (ps.K[3 + i] - v * ps.K[6 + i])) * iw;
        const double res = alpha * u + beta * v + gamma;
        const double K2[3] = {ps.K[6], ps.K[7], ps.K[8]};
        cvxr::cross(yc, q, j);
        cvxr::cross(yc, K2, k);
        CVX_UNROLL for (int i = 0; i < 3; ++i) { j[3 + i] = q[i]; k[3 + i] = K2[i]; }
        // J J^T - (rho / h_2) (k J^T + J k^T)  =  j (j - n)^T - n j^T,  n = (rho / h_2) k
        const double r2 = res * iw;
        double m[6], n[6];
        CVX_UNROLL for (int i = 0; i < 6; ++i) { n[i] = r2 * k[i]; m[i] = j[i] - n[i]; }
        int idx = 0;
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int l = i; l < 6; ++l) a[idx++] += j[i] * m[l] - n[i] * j[l];
        // rho S_ww
        const double qy = dot3(q, yc);
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            CVX_UNROLL for (int l = i; l < 3; ++l) a[cvxr::uidx(i, l)] += res * (0.5 * (q[i] * yc[l] + yc[i] * q[l]) - (i == l ? qy : 0.0));
        double j2 = 0.0;
        CVX_UNROLL for (int i = 0; i < 6; ++i) { a[21 + i] += j[i] * res; j2 += j[i] * j[i]; }
        a[27] += front ? sqrt(j2) * fabs(res) : INFINITY;
    }
}

// the gradients of record k (written as zeros when it is not live or the problem is not differentiated); nothing for k beyond the problem
CVX_HD void rec_grad(const Rec &r, const Prob &pb, int64_t k, const Pose &ps, const double *psi, bool zero, const Grads &g)
{
    if (k >= (int64_t)pb.n_p + pb.n_l) return;
    double xa0 = 0.0, xa1 = 0.0, xa2 = 0.0, xb0 = 0.0, xb1 = 0.0, xb2 = 0.0, s0 = 0.0, s1 = 0.0, Ga = 0.0, Gb = 0.0;
    const bool live = !zero && r.kind != 0;
    if (live) {
        CVX_ROLLED for (int s = 0; s < 2; ++s) {
            double X[3], alpha, beta, gamma, yc[3], u, v, iw;
            cvxr::rec_step(r, s, X, alpha, beta, gamma);
            cvxr::project(ps, X, yc, u, v, iw);
            double q[3], e[3], qa[3], d[3], ku[3], kv[3];
            const double K2[3] = {ps.K[6], ps.K[7], ps.K[8]};
            CVX_UNROLL for (int i = 0; i < 3; ++i) {
                ku[i] = (ps.K[i] - u * K2[i]) * iw;
                kv[i] = (ps.K[3 + i] - v * K2[i]) * iw;
                q[i] = alpha * ku[i] + beta * kv[i];
            }
            const double res = alpha * u + beta * v + gamma;
            cvxr::cross(psi, yc, e); // a x y + b'
            CVX_UNROLL for (int i = 0; i < 3; ++i) e[i] += psi[3 + i];
            const double sv = dot3(q, e), k2e = dot3(K2, e);
            cvxr::cross(q, psi, qa);
            // d (rho s) / dY-side = s q + rho (Q e + q x a),  Q e = -(K_2 s + q (K_2 . e)) / h_2
            CVX_UNROLL for (int i = 0; i < 3; ++i) d[i] = sv * q[i] + res * (qa[i] - iw * (K2[i] * sv + q[i] * k2e));
            const double x0 = -(ps.R[0] * d[0] + ps.R[3] * d[1] + ps.R[6] * d[2]);
            const double x1 = -(ps.R[1] * d[0] + ps.R[4] * d[1] + ps.R[7] * d[2]);
            const double x2 = -(ps.R[2] * d[0] + ps.R[5] * d[1] + ps.R[8] * d[2]);
            const bool far = r.kind == 2 && s == 1; // the second end point of a line
            xa0 += far ? 0.0 : x0; xa1 += far ? 0.0 : x1; xa2 += far ? 0.0 : x2;
            xb0 += far ? x0 : 0.0; xb1 += far ? x1 : 0.0; xb2 += far ? x2 : 0.0;
            s0 = s == 0 ? sv : s0;
            s1 = s == 1 ? sv : s1;
            // d (rho s) / d (alpha, beta); / d gamma is s
            Ga += u * sv + res * dot3(ku, e);
            Gb += v * sv + res * dot3(kv, e);
        }
    }
    if (k < pb.n_p) {
        // a point is the steps (1, 0, -x) and (0, 1, -y): d (rho s) / dx = -s_0, so dL/dx = +s_0
        if (g.p2) { g.p2[2 * k] = s0; g.p2[2 * k + 1] = s1; }
        if (g.p3) { g.p3[3 * k] = xa0; g.p3[3 * k + 1] = xa1; g.p3[3 * k + 2] = xa2; }
    } else {
        const int64_t kl = k - pb.n_p;
        if (g.l3) {
            double *o = g.l3 + 6 * kl;
            o[0] = xa0; o[1] = xa1; o[2] = xa2; o[3] = xb0; o[4] = xb1; o[5] = xb2;
        }
        if (g.l2) {
            double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
            if (live) {
                // through l = m / hypot(m_0, m_1), m = (a, 1) x (b, 1) = (a_1 - b_1, b_0 - a_0, a_0 b_1 - a_1 b_0)
                const double *x = pb.l2 + 4 * kl;
                const double a0 = x[0], a1 = x[1], b0 = x[2], b1 = x[3];
                const double inv = 1.0 / hypot(a1 - b1, b0 - a0);
                const double Gc = s0 + s1, Gl = Ga * r.q[0] + Gb * r.q[1] + Gc * r.q[2];
                const double m0 = (Ga - Gl * r.q[0]) * inv, m1 = (Gb - Gl * r.q[1]) * inv, m2 = Gc * inv;
                o0 = m1 - b1 * m2; o1 = b0 * m2 - m0; o2 = a1 * m2 - m1; o3 = m0 - a0 * m2;
            }
            double *o = g.l2 + 4 * kl;
            o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
        }
    }
}

// The whole backward pass of one problem over the lanes LN of refine_core.h (each / sum<N>).  first, stride: the records each() hands this
// lane are first, first + stride, ... in that order.  gR [9] / gt [3] may be null (zero).  write: this lane stores its records' gradients
// (false for a group that shadows another's problem).  Every lane of the problem returns the same status; info [2] (may be null) is
// stored by the lanes that pass a pointer: |g| / sum |J| |rho| and the smallest L_jj^2 / H_jj of the factorisation, NaN where the sums
// were not taken to the end.
template <class LN>
CVX_HD int vjp_problem(LN &ln, int first, int stride, const double *Kp, const double *Rin, const double *tin, const double *gR, const double *gt,
                       bool admit, bool write, const Grads &g, double *info)
{
    Pose ps;
    double t0[3];
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = Rin[i]; }
    CVX_UNROLL for (int i = 0; i < 3; ++i) t0[i] = tin[i];
    bool fin = true;
    CVX_UNROLL for (int i = 0; i < 9; ++i) fin = fin && cvxr::finite(ps.R[i]);
    CVX_UNROLL for (int i = 0; i < 3; ++i) fin = fin && cvxr::finite(t0[i]);
    const double det = ps.R[0] * (ps.R[4] * ps.R[8] - ps.R[5] * ps.R[7]) - ps.R[1] * (ps.R[3] * ps.R[8] - ps.R[5] * ps.R[6]) +
                       ps.R[2] * (ps.R[3] * ps.R[7] - ps.R[4] * ps.R[6]);
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const Rec &r) { cvxr::rec_centre(r, s5); });
    ln.template sum<5>(s5);
    const int n_live = (int)s5[4];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s5[3] > 0.0 ? s5[i] / s5[3] : 0.0;
    double Rc[3];
    cvxr::rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t0[i];

    // first pass: H, g and the scale of g
    double acc[ACC_N];
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
    ln.each([&](const Rec &r) { rec_acc_full(r, ps, acc); });
    ln.template sum<ACC_N>(acc);
    CVX_PHASE();

    int st = RVJP_OK;
    if (!admit || !fin || !(det > 0.0)) st = RVJP_SKIPPED;
    else if (n_live < 3) st = RVJP_SINGULAR;
    else if (!(acc[27] < INFINITY)) st = RVJP_BEHIND; // (a NaN or inf among the live records' numbers ends here too)
    double psi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double i0 = NAN, i1 = NAN;
    if (st == RVJP_OK) {
        // b in the centred chart: M^T (b_w, g_t)
        double G[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g_t[3] = {0.0, 0.0, 0.0};
        if (gR) CVX_UNROLL for (int i = 0; i < 9; ++i) G[i] = gR[i];
        if (gt) CVX_UNROLL for (int i = 0; i < 3; ++i) g_t[i] = gt[i];
        double M[9]; // G_R R^T
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            CVX_UNROLL for (int l = 0; l < 3; ++l) M[3 * i + l] = G[3 * i] * ps.R[3 * l] + G[3 * i + 1] * ps.R[3 * l + 1] + G[3 * i + 2] * ps.R[3 * l + 2];
        double gRc[3];
        cvxr::cross(g_t, Rc, gRc);
        const double b[6] = {M[7] - M[5] + gRc[0], M[2] - M[6] + gRc[1], M[3] - M[1] + gRc[2], g_t[0], g_t[1], g_t[2]};
        double A[36], Lm[36], x[6];
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int l = 0; l < 6; ++l) A[i * 6 + l] = acc[cvxr::uidx(i, l)];
        bool ok = cvxr::chol6(A, Lm);
        cvxr::chol6_solve(Lm, b, x);
        double gn = 0.0, ratio = INFINITY;
        CVX_UNROLL for (int i = 0; i < 6; ++i) {
            gn += acc[21 + i] * acc[21 + i];
            const double rr = 1.0 / (Lm[i * 6 + i] * Lm[i * 6 + i] * A[i * 6 + i]); // (the diagonal of Lm holds 1 / L_jj)
            ratio = rr < ratio ? rr : ratio;                                          // (a NaN never replaces a number: ok says what happened)
        }
        i0 = sqrt(gn) / (acc[27] + 1e-300);
        i1 = ok ? ratio : NAN;
        bool xfin = true;
        CVX_UNROLL for (int i = 0; i < 6; ++i) xfin = xfin && cvxr::finite(x[i]);
        if (!ok) st = RVJP_SINGULAR;          // not positive definite: the pose is not a strict minimum
        else if (!xfin) st = RVJP_BEHIND;     // a non-finite upstream gradient
        else CVX_UNROLL for (int i = 0; i < 6; ++i) psi[i] = x[i];
    }
    if (info) { info[0] = i0; info[1] = i1; }
    CVX_PHASE();

    // second pass: every record's gradients, by the lane that owns it
    if (write) {
        int64_t k = first; // (int64: k + stride may pass 2^31)
        const bool zero = st != RVJP_OK;
        ln.each([&](const Rec &r) {
            rec_grad(r, ln.pb, k, ps, psi, zero, g);
            k += stride;
        });
    }
    return st;
}

} // namespace cvxrg
