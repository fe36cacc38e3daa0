// refine_robust_vjp_core.h -- the backward pass of a robustly refined pose: implicit-function VJP of the minimum of sum w rho, host and
// device from one source.  Included, not edited: refine_core.h (records, steps, the projection, the chart, the
// Cholesky), refine_robust_core.h (the loss, a record's weight, s_k, the lane interface with the weight and the index beside each
// record) and refine_vjp_core.h (the least-squares backward pass whose quantities are reused here); the device's lanes (refine_lanes.h,
// a HIP header) come in through refine_robust_vjp_kernel.h, so that this file also compiles for the host alone.
//
// F = 1/2 sum_k w_k rho(s_k),  s_k = sum_i r_i^2 over the steps i of record k (refine_robust_core.h).  With refine_vjp_core.h's J, and
// v_k = sum_i J_i r_i,  omega_k = w_k rho'(s_k):
//   g = sum_k omega_k v_k,
//   H = sum_k omega_k H_k + 2 sum_k w_k rho''(s_k) v_k v_k^T,     H_k = sum_i J J^T + r (E^T Q E + S) the FULL per-record Hessian of
//   refine_vjp_core.h; the rank-one term is the one the forward iteration drops (Triggs' form) and the implicit function theorem needs.
//   rho'':  l2 0;  huber 0 for s <= delta^2, -delta / (2 s sqrt(s)) above;  cauchy -(1 / delta^2) / (1 + s / delta^2)^2.
// b and psi = H^-1 b are refine_vjp_core.h's, in the chart about the UNWEIGHTED mean of the live records.  With sigma_i = q_i . e_i
// (refine_vjp_core.h's s) and T_k = sum_i r_i sigma_i,  psi . g = sum_k w_k rho'(s_k) T_k,  so for an input theta of record k
//   dL/dtheta = -[ omega_k dT_k/dtheta + 2 w_k rho''(s_k) T_k sum_i r_i dr_i/dtheta ],       dL/dw_k = -rho'(s_k) T_k.
// Both terms are linear in what refine_vjp_core.h's rec_grad accumulates per step, so ONE set of accumulators serves: a light pass over
// the record's steps gives s_k and T_k, hence c1 = omega_k and c2 = 2 w_k rho''(s_k) T_k, and the full pass then accumulates
// c1 d(r sigma) + c2 r dr.   A record that is not live -- masked, a = b, or w_k = 0 -- is not read and gets exact zeros, its weight too.
#pragma once
#include "refine_core.h"
#include "refine_robust_core.h"
#include "refine_vjp_core.h"

namespace cvxrbg {

using cvxr::Pose;
using cvxr::Prob;
using cvxr::Rec;
using cvxrb::Loss;
using cvxrb::WProb;
using cvxrg::Grads;
using cvxrg::dot3;

constexpr int ACC_N = cvxr::ACC_N; // [0,21) H (upper triangle, row by row), [21,27) g, [27] sum omega |J| |r| (infinite when a live record has depth <= 0)

// rho'(s) and rho''(s); the branch rule is rho_prime's
CVX_HD void rho_d12(const Loss &l, double s, double &d1, double &d2)
{
    d1 = cvxrb::rho_prime(l, s);
    d2 = l.cauchy ? -l.inv_d2 * d1 * d1 : (s <= l.d2 ? 0.0 : -0.5 * d1 / s);
}

// The sums of one record at the pose (nothing for a record that is not live).  A step's residual and its gradient q are linear in the
// step's (alpha, beta, gamma), so scaling the three by sqrt(omega) turns refine_vjp_core.h's rec_acc_full into the omega-weighted sums
// with no product added to its 28 accumulations (omega = 1: its arithmetic bit for bit); the record's own share of g is kept aside for
// the rank-one term once both steps have given it:  2 w rho'' v v^T = (2 w rho'' / omega^2) (omega v) (omega v)^T.
CVX_HD void wrec_acc_full(const Rec &r, double w, const Pose &ps, const Loss &l, double *a)
{
    if (r.kind == 0) return;
    bool front_both;
    const double sk = cvxrb::rec_sq(r, ps, front_both);
    double d1, d2;
    rho_d12(l, sk, d1, d2);
    const double om = w * d1, so = sqrt(om);
    double gk[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    CVX_ROLLED for (int s = 0; s < 2; ++s) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        cvxr::rec_step(r, s, X, alpha, beta, gamma);
        alpha *= so; beta *= so; gamma *= so;
        const bool front = cvxr::project(ps, X, yc, u, v, iw);
        double j[6], k[6], q[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            q[i] = (alpha * (ps.K[i] - u * ps.K[6 + i]) + beta * (ps.K[3 + i] - v * ps.K[6 + i])) * iw;
        const double res = alpha * u + beta * v + gamma;
        const double K2[3] = {ps.K[6], ps.K[7], ps.K[8]};
        cvxr::cross(yc, q, j);
        cvxr::cross(yc, K2, k);
        CVX_UNROLL for (int i = 0; i < 3; ++i) { j[3 + i] = q[i]; k[3 + i] = K2[i]; }
        // J J^T - (r / h_2) (k J^T + J k^T)  =  j (j - n)^T - n j^T,  n = (r / h_2) k
        const double r2 = res * iw;
        double m[6], n[6];
        CVX_UNROLL for (int i = 0; i < 6; ++i) { n[i] = r2 * k[i]; m[i] = j[i] - n[i]; }
        int idx = 0;
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int c = i; c < 6; ++c) a[idx++] += j[i] * m[c] - n[i] * j[c];
        // r S_ww
        const double qy = dot3(q, yc);
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            CVX_UNROLL for (int c = i; c < 3; ++c) a[cvxr::uidx(i, c)] += res * (0.5 * (q[i] * yc[c] + yc[i] * q[c]) - (i == c ? qy : 0.0));
        double j2 = 0.0;
        CVX_UNROLL for (int i = 0; i < 6; ++i) { gk[i] += j[i] * res; j2 += j[i] * j[i]; }
        a[27] += front ? sqrt(j2) * fabs(res) : INFINITY;
    }
    const double c2 = 2.0 * w * d2 / (om * om); // (rho' > 0 for every finite s; an s that is not finite ends in a[27])
    int idx = 0;
    CVX_UNROLL for (int i = 0; i < 6; ++i) {
        const double cv = c2 * gk[i];
        CVX_UNROLL for (int c = i; c < 6; ++c) a[idx++] += cv * gk[c];
        a[21 + i] += gk[i];
    }
}

// The gradients of record k and of its weight (zeros when it is not live or the problem is not differentiated); nothing for k beyond
// the problem.  wp.ow_p / wp.ow_l are where the weight gradients of the problem's points / lines go (null: not wanted).
CVX_HD void wrec_grad(const Rec &r, double w, const WProb &wp, int64_t k, const Pose &ps, const double *psi, const Loss &l, bool zero, const Grads &g)
{
    const Prob &pb = wp.pb;
    if (k >= (int64_t)pb.n_p + pb.n_l) return;
    double xa0 = 0.0, xa1 = 0.0, xa2 = 0.0, xb0 = 0.0, xb1 = 0.0, xb2 = 0.0, s0 = 0.0, s1 = 0.0, Ga = 0.0, Gb = 0.0, gw = 0.0;
    const bool live = !zero && r.kind != 0;
    if (live) {
        const double K2[3] = {ps.K[6], ps.K[7], ps.K[8]};
        // the light pass: s_k and T_k
        double sk = 0.0, Tk = 0.0;
        CVX_ROLLED for (int s = 0; s < 2; ++s) {
            double X[3], alpha, beta, gamma, yc[3], u, v, iw, q[3], e[3];
            cvxr::rec_step(r, s, X, alpha, beta, gamma);
            cvxr::project(ps, X, yc, u, v, iw);
            CVX_UNROLL for (int i = 0; i < 3; ++i)
                q[i] = (alpha * (ps.K[i] - u * K2[i]) + beta * (ps.K[3 + i] - v * K2[i])) * iw;
            const double res = alpha * u + beta * v + gamma;
            cvxr::cross(psi, yc, e);
            CVX_UNROLL for (int i = 0; i < 3; ++i) e[i] += psi[3 + i];
            sk += res * res;
            Tk += res * dot3(q, e);
        }
        double d1, d2;
        rho_d12(l, sk, d1, d2);
        const double c1 = w * d1, c2 = 2.0 * w * d2 * Tk;
        gw = -d1 * Tk;
        CVX_ROLLED for (int s = 0; s < 2; ++s) {
            double X[3], alpha, beta, gamma, yc[3], u, v, iw;
            cvxr::rec_step(r, s, X, alpha, beta, gamma);
            cvxr::project(ps, X, yc, u, v, iw);
            double q[3], e[3], qa[3], d[3], ku[3], kv[3];
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
            // c1 d (r sigma) / dY + c2 r dr / dY:  d (r sigma) / dY = sigma q + r (Q e + q x a)  (refine_vjp_core.h),  dr / dY = q
            const double sc = c1 * sv + c2 * res, rc = c1 * res; // (sc is also the combined derivative by gamma, and minus that by a 2D point's coordinate)
            CVX_UNROLL for (int i = 0; i < 3; ++i) d[i] = sc * q[i] + rc * (qa[i] - iw * (K2[i] * sv + q[i] * k2e));
            const double x0 = -(ps.R[0] * d[0] + ps.R[3] * d[1] + ps.R[6] * d[2]);
            const double x1 = -(ps.R[1] * d[0] + ps.R[4] * d[1] + ps.R[7] * d[2]);
            const double x2 = -(ps.R[2] * d[0] + ps.R[5] * d[1] + ps.R[8] * d[2]);
            const bool far = r.kind == 2 && s == 1; // the second end point of a line
            xa0 += far ? 0.0 : x0; xa1 += far ? 0.0 : x1; xa2 += far ? 0.0 : x2;
            xb0 += far ? x0 : 0.0; xb1 += far ? x1 : 0.0; xb2 += far ? x2 : 0.0;
            s0 = s == 0 ? sc : s0;
            s1 = s == 1 ? sc : s1;
            // by (alpha, beta):  dr = (u, v),  d (r sigma) = (u sigma + r ku . e,  v sigma + r kv . e)
            Ga += u * sc + rc * dot3(ku, e);
            Gb += v * sc + rc * dot3(kv, e);
        }
    }
    if (k < pb.n_p) {
        if (g.p2) { g.p2[2 * k] = s0; g.p2[2 * k + 1] = s1; }
        if (g.p3) { g.p3[3 * k] = xa0; g.p3[3 * k + 1] = xa1; g.p3[3 * k + 2] = xa2; }
        if (wp.ow_p) wp.ow_p[k] = gw;
    } else {
        const int64_t kl = k - pb.n_p;
        if (g.l3) {
            double *o = g.l3 + 6 * kl;
            o[0] = xa0; o[1] = xa1; o[2] = xa2; o[3] = xb0; o[4] = xb1; o[5] = xb2;
        }
        if (g.l2) {
            double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
            if (live) {
                // through l = m / hypot(m_0, m_1), m = (a, 1) x (b, 1)  (refine_vjp_core.h)
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
        if (wp.ow_l) wp.ow_l[kl] = gw;
    }
}

// The whole backward pass of one problem over refine_robust_core.h's lanes (each hands f(const Rec &, double w, int64_t k); sum<N>).
// gR [9] / gt [3] may be null (zero).  write: this lane stores its records' gradients (false for a group that shadows another's
// problem).  Every lane of the problem returns the same status (refine_vjp_core.h's; RVJP_BEHIND also for a weight that is negative or
// not finite on a record its mask admits); the checks come in refine_robust_core.h's order.  info [2] (may be null) is stored by the lanes
// that pass a pointer: |g| / sum omega |J| |r| and the smallest L_jj^2 / H_jj, NaN where the sums were not taken to the end.
template <class LN>
CVX_HD int robust_vjp_problem(LN &ln, const WProb &wp, const double *Kp, const double *Rin, const double *tin, const double *gR, const double *gt,
                              bool admit, bool write, const Loss &l, const Grads &g, double *info)
{
    using namespace cvxrg;
    Pose ps;
    double t0[3];
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = Rin[i]; }
    CVX_UNROLL for (int i = 0; i < 3; ++i) t0[i] = tin[i];
    bool fin = true;
    CVX_UNROLL for (int i = 0; i < 9; ++i) fin = fin && cvxr::finite(ps.R[i]);
    CVX_UNROLL for (int i = 0; i < 3; ++i) fin = fin && cvxr::finite(t0[i]);
    const double det = ps.R[0] * (ps.R[4] * ps.R[8] - ps.R[5] * ps.R[7]) - ps.R[1] * (ps.R[3] * ps.R[8] - ps.R[5] * ps.R[6]) +
                       ps.R[2] * (ps.R[3] * ps.R[7] - ps.R[4] * ps.R[6]);
    double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const Rec &r, double w, int64_t) { cvxrb::wrec_centre(r, w, s6); });
    ln.template sum<6>(s6);
    const int n_live = (int)s6[4];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s6[3] > 0.0 ? s6[i] / s6[3] : 0.0;
    double Rc[3];
    cvxr::rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t0[i];

    // first pass: H, g and the scale of g
    double acc[ACC_N];
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
    ln.each([&](const Rec &r, double w, int64_t) { wrec_acc_full(r, w, ps, l, acc); });
    ln.template sum<ACC_N>(acc);
    CVX_PHASE();

    int st = RVJP_OK;
    if (!admit || !fin || !(det > 0.0)) st = RVJP_SKIPPED;
    else if (s6[5] > 0.0) st = RVJP_BEHIND; // a weight that is negative or not finite
    else if (n_live < 3) st = RVJP_SINGULAR;
    else if (!(acc[27] < INFINITY)) st = RVJP_BEHIND; // (a NaN or inf among the live records' numbers ends here too)
    double psi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double i0 = NAN, i1 = NAN;
    if (st == RVJP_OK) {
        // b in the centred chart: M^T (b_w, g_t)  (refine_vjp_core.h)
        double G[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g_t[3] = {0.0, 0.0, 0.0};
        if (gR) CVX_UNROLL for (int i = 0; i < 9; ++i) G[i] = gR[i];
        if (gt) CVX_UNROLL for (int i = 0; i < 3; ++i) g_t[i] = gt[i];
        double M[9]; // G_R R^T
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            CVX_UNROLL for (int c = 0; c < 3; ++c) M[3 * i + c] = G[3 * i] * ps.R[3 * c] + G[3 * i + 1] * ps.R[3 * c + 1] + G[3 * i + 2] * ps.R[3 * c + 2];
        double gRc[3];
        cvxr::cross(g_t, Rc, gRc);
        const double b[6] = {M[7] - M[5] + gRc[0], M[2] - M[6] + gRc[1], M[3] - M[1] + gRc[2], g_t[0], g_t[1], g_t[2]};
        double A[36], Lm[36], x[6];
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int c = 0; c < 6; ++c) A[i * 6 + c] = acc[cvxr::uidx(i, c)];
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
        if (!ok) st = RVJP_SINGULAR;          // not positive definite: the pose is not a strict minimum of the robust cost
        else if (!xfin) st = RVJP_BEHIND;     // a non-finite upstream gradient
        else CVX_UNROLL for (int i = 0; i < 6; ++i) psi[i] = x[i];
    }
    if (info) { info[0] = i0; info[1] = i1; }
    CVX_PHASE();

    // second pass: every record's gradients and its weight's, by the lane that owns it
    if (write) {
        const bool zero = st != RVJP_OK;
        ln.each([&](const Rec &r, double w, int64_t k) { wrec_grad(r, w, wp, k, ps, psi, l, zero, g); });
    }
    return st;
}

} // namespace cvxrbg
