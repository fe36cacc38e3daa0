// refine_core.h -- reprojection refinement of a pose: Levenberg-Marquardt on PIXEL residuals, host and device from one source
// (DESIGN.md section 15).  The solver, its VJP and the RANSAC refits minimise the reference's algebraic cost; this polishes their pose
// on the quantity the RANSAC layers judge it by.
//
// Residuals (pixels).  With Y = R X + t, (h0, h1, h2) = K Y and (u, v) = (h0 / h2, h1 / h2):
//   a point (x, y) <-> X gives (u - x, v - y);
//   a line (a, b) <-> (E0, E1) gives l . (u_k, v_k, 1) for both end points E_k, l = (a, 1) x (b, 1) / hypot(l_0, l_1): the signed distance
//   of the projected end point from the image line, the quantity of cvxnl::image_line / end_point_near.
// A correspondence is LIVE when its mask byte is absent or non-zero; a 2D line with a = b is not live.  A record that is not live is not
// read (points) or not read beyond its 2D samples (lines), so whatever it holds cannot reach the result.  depth = Y_z.
//
// Chart.  Internally the pose is perturbed about the mean c of the live 3D records, as vjp_core.h does about its centre:
//   X -> exp([w]x) R (X - c) + tc + tau_c,   tc = R c + t,   yc = R (X - c).
// One residual row with pixel-space gradient q (d residual / d Y) is then  J = [yc x q, q].  The public chart is R' = exp([w]x) R,
// t' = t + tau; to first order tau = tau_c + (R c) x w, which is how the step norm and the covariance are brought to it.
//
// Schedule (fixed: host, device and the test reference run the same one).  lambda_0 = 1e-3; solve (J^T J + lambda diag(J^T J)) d = -J^T r
// by Cholesky; the trial pose is accepted iff every live record has depth > 0 and cost_trial <= cost; accept: lambda <- max(lambda / 10,
// 1e-12), reject: lambda <- 10 lambda, and lambda > 1e12 ends the run with what was reached.  CONVERGED: an accepted step with
// |d| <= step_tol (1 + |t|) in the public chart.  One addition, for poses that have reached the rounding floor of the cost: a trial at
// lambda <= lambda_0 (a step that damping has not shortened) whose cost differs from the current one by no more than COST_TOL of it --
// accepted or rejected -- or a rejected one whose step is below the step tolerance, ends the run as CONVERGED at the pose reached.  There the two costs agree to the rounding of their sums,
// whether the trial compares <= is chance, and without the rule a converged pose spends a dozen rejected trials raising lambda until a
// step is short enough to win the toss (a step of 1e-9 along a weak direction changes a cost of 20 by 1e-15).  Every trial counts as an
// iteration.
#pragma once
#include <math.h>
#include <stdint.h>

#include "problem_io.h"

#if defined(__HIPCC__)
#define CVX_ROLLED _Pragma("unroll 1")
#else
#define CVX_ROLLED
#endif
// Between the phases of an iteration on the device: the instruction scheduler does not move code across.  Left to itself it interleaves
// the reduction, the factorisation and the pose update until their temporaries together exceed the register file.
#if defined(__HIP_DEVICE_COMPILE__)
#define CVX_PHASE() __builtin_amdgcn_sched_barrier(0)
#else
#define CVX_PHASE() ((void)0)
#endif

namespace cvxr {

enum RefineStatus : int { REFINE_CONVERGED = 0, REFINE_MAXITER = 1, REFINE_SKIPPED = 2, REFINE_SINGULAR = 3, REFINE_BEHIND = 4 };

constexpr int ACC_N = 28;           // doubles reduced per evaluation: [0,21) J^T J (upper triangle, row by row), [21,27) J^T r, [27] cost (infinite when a live record has depth <= 0)
constexpr double PIVOT_TOL = 1e-11; // Cholesky pivot below this fraction of its diagonal entry: not positive definite
constexpr double LAMBDA_MIN = 1e-12, LAMBDA_MAX = 1e12;
constexpr double COST_TOL = 1e-12;  // a rejected trial within this fraction of the current cost: the rounding floor (see above)

struct Opts {
    int max_iters;
    double step_tol, lambda0, sigma_px;
};

// one problem's correspondences: n_p points then n_l lines, masks optional
struct Prob {
    int n_p, n_l;
    const double *p2, *p3, *l2, *l3;
    const uint8_t *mp, *ml;
};

// a correspondence as the iteration sees it: kind 0 not live, 1 point (p = X, q = (x, y)), 2 line (p = E0 E1, q = normalised image line)
struct Rec {
    double p[6], q[3];
    int kind;
};

// (Every field is assigned once, after the branches, from scalars: stores to different fields in the two branches get merged into one
// store through a computed address, which keeps the whole record -- and the lanes' register copy of it -- in scratch memory.)
CVX_HD void rec_load(const Prob &pb, int k, Rec &r)
{
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0, p5 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    int kind = 0;
    if (k < pb.n_p) {
        if (!pb.mp || pb.mp[k]) {
            const double *X = pb.p3 + 3 * (int64_t)k, *x = pb.p2 + 2 * (int64_t)k;
            p0 = X[0]; p1 = X[1]; p2 = X[2];
            q0 = x[0]; q1 = x[1];
            kind = 1;
        }
    } else if (k < pb.n_p + pb.n_l) {
        const int kl = k - pb.n_p;
        if (!pb.ml || pb.ml[kl]) {
            const double *x = pb.l2 + 4 * (int64_t)kl;
            const double l0 = x[1] - x[3], l1 = x[2] - x[0], l2 = x[0] * x[3] - x[1] * x[2];
            const double hyp = hypot(l0, l1);
            if (hyp != 0.0) { // (a = b: no image line)
                const double inv = 1.0 / hyp;
                const double *E = pb.l3 + 6 * (int64_t)kl;
                p0 = E[0]; p1 = E[1]; p2 = E[2]; p3 = E[3]; p4 = E[4]; p5 = E[5];
                q0 = l0 * inv; q1 = l1 * inv; q2 = l2 * inv;
                kind = 2;
            }
        }
    }
    r.p[0] = p0; r.p[1] = p1; r.p[2] = p2; r.p[3] = p3; r.p[4] = p4; r.p[5] = p5;
    r.q[0] = q0; r.q[1] = q1; r.q[2] = q2;
    r.kind = kind;
}

struct Pose {
    double K[9], R[9], tc[3], c[3];
};

// (not x - x == 0: where x is a product, the device contracts the difference into one fused multiply-add, which returns the ROUNDING ERROR
// of the product -- not zero -- and every finite step was taken for non-finite)
CVX_HD bool finite(double x) { return fabs(x) < INFINITY; }

CVX_HD void cross(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

CVX_HD void rot_c(const Pose &ps, double *Rc)
{
    CVX_UNROLL for (int i = 0; i < 3; ++i) Rc[i] = ps.R[3 * i] * ps.c[0] + ps.R[3 * i + 1] * ps.c[1] + ps.R[3 * i + 2] * ps.c[2];
}

// pixel (u, v) of X, yc = R (X - c); true when the depth is positive (false for NaN)
CVX_HD bool project(const Pose &ps, const double *X, double *yc, double &u, double &v, double &iw)
{
    const double d[3] = {X[0] - ps.c[0], X[1] - ps.c[1], X[2] - ps.c[2]};
    double Y[3];
    CVX_UNROLL for (int i = 0; i < 3; ++i) {
        yc[i] = ps.R[3 * i] * d[0] + ps.R[3 * i + 1] * d[1] + ps.R[3 * i + 2] * d[2];
        Y[i] = yc[i] + ps.tc[i];
    }
    const double h0 = ps.K[0] * Y[0] + ps.K[1] * Y[1] + ps.K[2] * Y[2];
    const double h1 = ps.K[3] * Y[0] + ps.K[4] * Y[1] + ps.K[5] * Y[2];
    const double h2 = ps.K[6] * Y[0] + ps.K[7] * Y[1] + ps.K[8] * Y[2];
    iw = 1.0 / h2;
    u = h0 * iw;
    v = h1 * iw;
    return Y[2] > 0.0;
}

// A record is up to two STEPS, each one residual  alpha u + beta v + gamma  of one projected 3D point: a point is (1, 0, -x) and (0, 1, -y)
// of X, a line is l of E0 and l of E1.  The steps are taken by selects inside a rolled loop, so that a pass holds ONE copy of the
// projection and of the 28 accumulations per record, whatever its kind.
CVX_HD void rec_step(const Rec &r, int s, double *X, double &alpha, double &beta, double &gamma)
{
    const bool pt = r.kind == 1, second = s == 1;
    const double a0 = r.p[0], a1 = r.p[1], a2 = r.p[2], b0 = r.p[3], b1 = r.p[4], b2 = r.p[5];
    const bool far = !pt && second;
    X[0] = far ? b0 : a0; X[1] = far ? b1 : a1; X[2] = far ? b2 : a2;
    alpha = pt ? (second ? 0.0 : 1.0) : r.q[0];
    beta = pt ? (second ? 1.0 : 0.0) : r.q[1];
    gamma = pt ? (second ? -r.q[1] : -r.q[0]) : r.q[2];
}

// the sums of one record at a pose (nothing for a record that is not live): J = [yc x q, q] with q = d residual / d Y
CVX_HD void rec_acc(const Rec &r, const Pose &ps, double *a)
{
    if (r.kind == 0) return;
    CVX_ROLLED for (int s = 0; s < 2; ++s) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        rec_step(r, s, X, alpha, beta, gamma);
        const bool front = project(ps, X, yc, u, v, iw);
        double j[6], q[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            q[i] = (alpha * (ps.K[i] - u * ps.K[6 + i]) + beta * (ps.K[3 + i] - v * ps.K[6 + i])) * iw;
        const double res = alpha * u + beta * v + gamma;
        cross(yc, q, j);
        j[3] = q[0]; j[4] = q[1]; j[5] = q[2];
        int idx = 0;
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int k = i; k < 6; ++k) a[idx++] += j[i] * j[k];
        CVX_UNROLL for (int i = 0; i < 6; ++i) a[21 + i] += j[i] * res;
        a[27] += front ? res * res : INFINITY;
    }
}

// cost of one record at a trial pose: squared residuals, infinite when its depth is not positive
CVX_HD void rec_cost(const Rec &r, const Pose &ps, double *c1)
{
    if (r.kind == 0) return;
    CVX_ROLLED for (int s = 0; s < 2; ++s) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        rec_step(r, s, X, alpha, beta, gamma);
        const bool front = project(ps, X, yc, u, v, iw);
        const double res = alpha * u + beta * v + gamma;
        c1[0] += front ? res * res : INFINITY;
    }
}

// centroid sums of the live 3D records: s[0..2] sum, s[3] records, s[4] live correspondences
CVX_HD void rec_centre(const Rec &r, double *s)
{
    if (r.kind == 1) {
        s[0] += r.p[0]; s[1] += r.p[1]; s[2] += r.p[2];
        s[3] += 1.0; s[4] += 1.0;
    } else if (r.kind == 2) {
        s[0] += r.p[0] + r.p[3]; s[1] += r.p[1] + r.p[4]; s[2] += r.p[2] + r.p[5];
        s[3] += 2.0; s[4] += 1.0;
    }
}

CVX_HD constexpr int uidx(int i, int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

// Cholesky A = L L^T of a full symmetric 6x6: the strict lower triangle of L in Lm, and on its diagonal the RECIPROCALS 1 / L_jj (the
// solves multiply); false when a pivot fails
CVX_HD bool chol6(const double *A, double *Lm)
{
    bool ok = true;
    CVX_UNROLL for (int i = 0; i < 36; ++i) Lm[i] = A[i];
    CVX_UNROLL for (int j = 0; j < 6; ++j) {
        double d = Lm[j * 6 + j];
        CVX_UNROLL for (int k = 0; k < j; ++k) d -= Lm[j * 6 + k] * Lm[j * 6 + k];
        ok = ok && (d > PIVOT_TOL * A[j * 6 + j]) && (d < 1.7e308);
        const double ri = 1.0 / sqrt(d);
        Lm[j * 6 + j] = ri;
        CVX_UNROLL for (int i = j + 1; i < 6; ++i) {
            double x = Lm[i * 6 + j];
            CVX_UNROLL for (int k = 0; k < j; ++k) x -= Lm[i * 6 + k] * Lm[j * 6 + k];
            Lm[i * 6 + j] = x * ri;
        }
        CVX_PHASE();
    }
    return ok;
}

CVX_HD void chol6_solve(const double *Lm, const double *b, double *x6)
{
    double y[6];
    CVX_UNROLL for (int i = 0; i < 6; ++i) {
        double x = b[i];
        CVX_UNROLL for (int k = 0; k < i; ++k) x -= Lm[i * 6 + k] * y[k];
        y[i] = x * Lm[i * 6 + i];
    }
    CVX_UNROLL for (int ii = 0; ii < 6; ++ii) {
        const int i = 5 - ii;
        double x = y[i];
        CVX_UNROLL for (int k = i + 1; k < 6; ++k) x -= Lm[k * 6 + i] * x6[k];
        x6[i] = x * Lm[i * 6 + i];
    }
}

// (J^T J + lambda diag(J^T J)) d = -J^T r; false (and d = 0) when the damped matrix is not positive definite or the step is not finite
CVX_HD bool damped_step(const double *a, double lambda, double *d)
{
    double A[36], Lm[36], b[6];
    CVX_UNROLL for (int i = 0; i < 6; ++i) {
        CVX_UNROLL for (int j = 0; j < 6; ++j) A[i * 6 + j] = a[uidx(i, j)];
        A[i * 6 + i] += lambda * a[uidx(i, i)];
        b[i] = -a[21 + i];
    }
    bool ok = chol6(A, Lm);
    double x[6];
    chol6_solve(Lm, b, x);
    CVX_UNROLL for (int i = 0; i < 6; ++i) ok = ok && finite(x[i]);
    CVX_UNROLL for (int i = 0; i < 6; ++i) d[i] = ok ? x[i] : 0.0;
    return ok;
}

// R <- exp([w]x) R, tc <- tc + tau.  exp([w]x) is the rotation of the unit quaternion (cos(th / 2), sin(th / 2) w / th), th = |w|: the half
// angle is scaled by 2^-5, its sine and cosine come from their Taylor polynomials (|x| <= 1/8 for th <= 8: truncation below 1e-17), five
// doublings bring them back, and the quaternion is normalised before use, so that what multiplies R is a rotation to rounding whatever th
// is.  (No libm call: the device's sin brings its argument reduction and some forty constants into the loop.)
CVX_HD void pose_step(Pose &ps, const double *d)
{
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double x2 = th2 * (0.25 / 1024.0); // (th / 2 / 32)^2
    // sin(x) / x and cos(x) in x^2
    double sc = 1.0 + x2 * (-1.0 / 6.0 + x2 * (1.0 / 120.0 + x2 * (-1.0 / 5040.0 + x2 * (1.0 / 362880.0 - x2 * (1.0 / 39916800.0)))));
    double c = 1.0 + x2 * (-0.5 + x2 * (1.0 / 24.0 + x2 * (-1.0 / 720.0 + x2 * (1.0 / 40320.0 + x2 * (-1.0 / 3628800.0 + x2 * (1.0 / 479001600.0))))));
    // doubling: sin(2x) / (2x) = (sin(x) / x) cos(x),  cos(2x) = 2 cos(x)^2 - 1 = 1 - 2 x^2 (sin(x) / x)^2 (the second form keeps the digits of a small angle)
    double xx = x2;
    CVX_UNROLL for (int k = 0; k < 5; ++k) {
        const double s2 = xx * sc * sc; // sin(x)^2
        sc = sc * c;
        c = 1.0 - 2.0 * s2;
        xx *= 4.0;
    }
    // q = (c, 0.5 sc w), |q| = 1 up to rounding and truncation
    const double qn = 1.0 / sqrt(c * c + 0.25 * sc * sc * th2);
    const double qw = c * qn, qx = 0.5 * sc * d[0] * qn, qy = 0.5 * sc * d[1] * qn, qz = 0.5 * sc * d[2] * qn;
    double E[9];
    E[0] = 1.0 - 2.0 * (qy * qy + qz * qz); E[1] = 2.0 * (qx * qy - qw * qz);       E[2] = 2.0 * (qx * qz + qw * qy);
    E[3] = 2.0 * (qx * qy + qw * qz);       E[4] = 1.0 - 2.0 * (qx * qx + qz * qz); E[5] = 2.0 * (qy * qz - qw * qx);
    E[6] = 2.0 * (qx * qz - qw * qy);       E[7] = 2.0 * (qy * qz + qw * qx);       E[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    double Rn[9];
    CVX_UNROLL for (int i = 0; i < 3; ++i)
        CVX_UNROLL for (int j = 0; j < 3; ++j) Rn[3 * i + j] = E[3 * i] * ps.R[j] + E[3 * i + 1] * ps.R[3 + j] + E[3 * i + 2] * ps.R[6 + j];
    CVX_UNROLL for (int i = 0; i < 9; ++i) ps.R[i] = Rn[i];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] += d[3 + i];
}

// |step| in the public chart over (1 + |t|)
CVX_HD double step_measure(const Pose &ps, const double *d)
{
    double Rc[3], x[3];
    rot_c(ps, Rc);
    cross(Rc, d, x); // (R c) x w
    double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], t2 = 0.0;
    CVX_UNROLL for (int i = 0; i < 3; ++i) {
        const double tau = d[3 + i] + x[i], t = ps.tc[i] - Rc[i];
        n2 += tau * tau;
        t2 += t * t;
    }
    return sqrt(n2) / (1.0 + sqrt(t2));
}

// cov [36] = sigma2 (J^T J)^-1 at the pose, brought to the public chart: xi_pub = M xi_c, M = [[I, 0], [S, I]], S = [R c]x, so that
// cov = sigma2 M (J^T J)^-1 M^T.  Column k is M y with (J^T J) y = M^T e_k: one Cholesky, six solves, each column stored as soon as it is
// known (a lane that does not write passes null), so that 36 doubles are never held.  NaN when J^T J is not positive definite.
CVX_HD void covariance(const double *a, const Pose &ps, double sigma2, bool valid, double *cov)
{
    double A6[36], Lm[36];
    CVX_UNROLL for (int i = 0; i < 6; ++i)
        CVX_UNROLL for (int j = 0; j < 6; ++j) A6[i * 6 + j] = a[uidx(i, j)];
    const bool ok = chol6(A6, Lm) && valid;
    double Rc[3];
    rot_c(ps, Rc);
    const double S[9] = {0.0, -Rc[2], Rc[1], Rc[2], 0.0, -Rc[0], -Rc[1], Rc[0], 0.0};
    CVX_UNROLL for (int k = 0; k < 6; ++k) {
        double m[6], y[6]; // row k of M
        CVX_UNROLL for (int i = 0; i < 6; ++i) m[i] = i == k ? 1.0 : 0.0;
        if (k >= 3) CVX_UNROLL for (int i = 0; i < 3; ++i) m[i] = S[3 * (k - 3) + i];
        chol6_solve(Lm, m, y);
        if (cov) {
            CVX_UNROLL for (int i = 0; i < 3; ++i) {
                cov[i * 6 + k] = ok ? sigma2 * y[i] : NAN;
                cov[(3 + i) * 6 + k] = ok ? sigma2 * (S[3 * i] * y[0] + S[3 * i + 1] * y[1] + S[3 * i + 2] * y[2] + y[3 + i]) : NAN;
            }
        }
    }
}

// status s admitted by mask: bit s
CVX_HD bool admitted(int status, uint32_t mask) { return status >= 0 && status < 32 && ((mask >> status) & 1u); }

// (cost before: stored by the writing lane as soon as it is known -- held to the end it is one more value that lives through the whole loop;
// R, t: valid when status <= REFINE_MAXITER, otherwise the caller passes the input pose through)
struct Result {
    double R[9], t[3], cost;
    int iters, status, n_live;
};

// The whole refinement of one problem, written once for the three ways its correspondences are spread over lanes.  LN provides
//   each(f)      f(const Rec &) for every record THIS lane owns;
//   sum<N>(v)    v[0 .. N) summed over the lanes of the problem, every lane receiving the same totals;
//   any(p)       p of any problem that shares this lane's control flow (the four groups of a wavefront; otherwise p itself).
// Every lane of a problem ends with the same Result; cost_before is stored by the lanes that pass a pointer.  Lanes whose problem has ended keep running the
// loop with their state frozen until any() releases them: the exchanges of sum() stay convergent.
template <class LN>
CVX_HD void refine_problem(LN &ln, const double *Kp, const double *Rin, const double *tin, bool admit, const Opts &o, Result &res, double *cost_before)
{
    Pose ps;
    double t0[3];
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = Rin[i]; }
    CVX_UNROLL for (int i = 0; i < 3; ++i) t0[i] = tin[i];
    bool fin = true;
    CVX_UNROLL for (int i = 0; i < 9; ++i) fin = fin && finite(ps.R[i]);
    CVX_UNROLL for (int i = 0; i < 3; ++i) fin = fin && finite(t0[i]);
    const double det = ps.R[0] * (ps.R[4] * ps.R[8] - ps.R[5] * ps.R[7]) - ps.R[1] * (ps.R[3] * ps.R[8] - ps.R[5] * ps.R[6]) +
                       ps.R[2] * (ps.R[3] * ps.R[7] - ps.R[4] * ps.R[6]);
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const Rec &r) { rec_centre(r, s5); });
    ln.template sum<5>(s5);
    const int n_live = (int)s5[4];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s5[3] > 0.0 ? s5[i] / s5[3] : 0.0;
    double Rc[3];
    rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t0[i];

    int st = -1; // running
    if (!admit || !fin || !(det > 0.0)) st = REFINE_SKIPPED;
    else if (n_live < 3) st = REFINE_SINGULAR;
    double acc[ACC_N];
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
    double cost = NAN, lambda = o.lambda0;
    if (cost_before) *cost_before = NAN;
    int iters = 0;
    bool active = st < 0;
    int seen = 0; // bit 0 SOLVED: some damped system was positive definite; bit 1 MOVED: some trial was accepted (one value, not two flags: on the device each is a register that lives through the loop)

    for (int it = 0;; ++it) {
        const bool run = ln.any(active) && it < o.max_iters; // another trial follows
        if (!run && it > 0) break;                           // nobody needs the sums any more
        // ONE site evaluates the sums, at the pose each problem has reached: the input pose, the pose after every trial (a rejected trial
        // leaves it where it was, and the sums are taken again: rejections are few)
        CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
        ln.each([&](const Rec &r) { rec_acc(r, ps, acc); });
        ln.template sum<ACC_N>(acc);
        if (it == 0 && active) {
            cost = acc[27];
            if (!(cost < INFINITY)) { st = REFINE_BEHIND; active = false; } // (a NaN or inf among the live records' numbers ends here too: the contract, see the header)
            else if (cost_before) *cost_before = cost;
        }
        if (!run) break;
        double d[6];
        const bool ok = damped_step(acc, lambda, d);
        CVX_PHASE();
        const double rel = step_measure(ps, d);
        Pose tr = ps;
        pose_step(tr, d);
        CVX_PHASE();
        double c1[1] = {0.0};
        ln.each([&](const Rec &r) { rec_cost(r, tr, c1); });
        ln.template sum<1>(c1);
        if (active) {
            ++iters;
            seen |= ok ? 1 : 0;
            const bool floor = lambda <= o.lambda0 && fabs(c1[0] - cost) <= COST_TOL * cost; // the two costs agree to their rounding
            if (ok && c1[0] <= cost) { // (a trial with a record behind the camera costs infinity)
                ps = tr;
                seen |= 2;
                cost = c1[0];
                lambda = lambda * 0.1 > LAMBDA_MIN ? lambda * 0.1 : LAMBDA_MIN;
                if (rel <= o.step_tol || floor) { st = REFINE_CONVERGED; active = false; }
            } else if (ok && c1[0] < INFINITY && ((rel <= o.step_tol && lambda <= o.lambda0) || floor)) {
                st = REFINE_CONVERGED; active = false; // (see the header: the rounding floor of the cost)
            } else {
                lambda *= 10.0;
                if (lambda > LAMBDA_MAX) { st = (seen & 1) ? REFINE_MAXITER : REFINE_SINGULAR; active = false; }
            }
        }
    }
    if (st < 0) st = REFINE_MAXITER;
    const bool done = st <= REFINE_MAXITER;
    if (!done && cost_before) *cost_before = NAN; // (lambda ran out before any system was positive definite)
    rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 9; ++i) res.R[i] = ps.R[i];
    // (a pose that no trial has moved is the input pose bit for bit -- max_iters = 0, or converged on a rejected trial: (R c + t) - R c is t
    // only to the rounding of |R c|, so t is read again; nothing has been written by now, the outputs may alias the inputs)
    CVX_UNROLL for (int i = 0; i < 3; ++i) res.t[i] = (seen & 2) ? ps.tc[i] - Rc[i] : tin[i];
    res.cost = done ? cost : NAN;
    res.iters = done ? iters : 0; res.status = st; res.n_live = n_live;
}

// The covariance of a refined pose, a pass of its own over the same lanes (kept out of refine_problem: its factorisation on top of the
// loop's state does not fit the register file): the sums at (R, t) about the same centre, then covariance().  status / cost_after / n_live
// are refine_problem's outputs; a pose that was not refined gets NaN.
template <class LN>
CVX_HD void covariance_problem(LN &ln, const double *Kp, const double *R, const double *t, int status, double cost_after, int n_live, const Opts &o, double *cov)
{
    Pose ps;
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = R[i]; }
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const Rec &r) { rec_centre(r, s5); });
    ln.template sum<5>(s5);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s5[3] > 0.0 ? s5[i] / s5[3] : 0.0;
    double Rc[3];
    rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t[i];
    double acc[ACC_N];
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
    ln.each([&](const Rec &r) { rec_acc(r, ps, acc); });
    ln.template sum<ACC_N>(acc);
    const int m = 2 * n_live;
    const double sigma2 = o.sigma_px > 0.0 ? o.sigma_px * o.sigma_px : (m > 6 ? cost_after / (double)(m - 6) : NAN);
    covariance(acc, ps, sigma2, status <= REFINE_MAXITER, cov);
}

// the host's lanes: one lane owns the whole problem
struct HostLanes {
    Prob pb;
    template <class F>
    void each(F f)
    {
        const int n = pb.n_p + pb.n_l;
        for (int k = 0; k < n; ++k) {
            Rec r;
            rec_load(pb, k, r);
            f(r);
        }
    }
    template <int N>
    void sum(double *) {}
    bool any(bool p) { return p; }
};

} // namespace cvxr
