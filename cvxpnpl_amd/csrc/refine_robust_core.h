// refine_robust_core.h -- reprojection refinement under a robust loss and per-correspondence weights, host and device from one source
// (DESIGN.md section 17).  refine_core.h minimises the plain sum of squared pixel residuals; this minimises
//   f = sum_k w_k rho(s_k),   s_k = r_{k,0}^2 + r_{k,1}^2  (both steps of correspondence k: a point's squared pixel distance, a line's
//   two squared end-point distances), w_k the caller's weight (1 when absent), rho one of
//     l2      rho = s                                         rho' = 1
//     huber   rho = s for s <= delta^2, 2 delta sqrt(s) - delta^2 above        rho' = 1, delta / sqrt(s) above
//     cauchy  rho = delta^2 log1p(s / delta^2)                rho' = 1 / (1 + s / delta^2)
// with the re-weighted normal equations  sum omega_k j j^T,  sum omega_k j r,  omega_k = w_k rho'(s_k) at the pose reached (Triggs'
// first-order form: the rho'' term is dropped), on the schedule of refine_core.h unchanged, run on the robust cost.  The weights are
// evaluated again at every pose at which the sums are taken; there is no inner loop.
//
// Everything a record, a pose and a step are is refine_core.h's: Rec, rec_load, rec_step, project, damped_step, pose_step, step_measure.
// New here: a record's weight, the pass that knows a record's s_k before it accumulates either of its steps, the cost pass, the loop
// around them and the pass that reports rho'(s_k) per record.
//
// LIVE: mask byte absent or non-zero, for a line a != b, and w_k != 0.  A zero weight is a mask: the record is not read.  A weight that
// is negative or not finite, in a record that its mask admits, ends the problem with status 4 (REFINE_BEHIND: the problem's numbers
// cannot be used), before the count of live records is looked at.
#pragma once
#include "refine_core.h"

namespace cvxrb {

using cvxr::Opts;
using cvxr::Pose;
using cvxr::Prob;
using cvxr::Rec;
using cvxr::Result;
using cvxr::ACC_N;

enum LossKind : int { LOSS_L2 = 0, LOSS_HUBER = 1, LOSS_CAUCHY = 2 };

// l2 is huber with delta = infinity: no record leaves the quadratic branch
struct Loss {
    int cauchy;
    double delta, d2, inv_d2;
};

CVX_HD Loss make_loss(int kind, double scale_px)
{
    Loss l;
    l.cauchy = kind == LOSS_CAUCHY;
    l.delta = kind == LOSS_L2 ? INFINITY : scale_px;
    l.d2 = kind == LOSS_L2 ? INFINITY : scale_px * scale_px;
    l.inv_d2 = kind == LOSS_L2 ? 0.0 : 1.0 / (scale_px * scale_px);
    return l;
}

// log1p(x) for x >= 0 (NaN and inf pass through), the algorithm of fdlibm's log1p: 1 + x = m 2^k with m in [sqrt(1/2), sqrt(2)), f = m - 1,
// log(1 + f) = f - f^2 / 2 + s (f^2 / 2 + R(s^2)), s = f / (2 + f), and the rounding of 1 + x brought back by c.  Error below 1 ulp.  One
// statement of it for host and device, with nine constants: the device library's log1p brings some forty into the loop, where they live in
// registers through every pass.
CVX_HD double log1p_pos(double x)
{
    const double u = 1.0 + x;
    int k;
    double m = frexp(u, &k); // [1/2, 1)
    const bool low = m < 0.70710678118654752440;
    m = low ? 2.0 * m : m;
    k = low ? k - 1 : k;
    const double f = k == 0 ? x : m - 1.0; // (k = 0: 1 + x is not needed, x itself is exact)
    const double c = k == 0 ? 0.0 : (x - (u - 1.0)) / u;
    const double hfsq = 0.5 * f * f, sv = f / (2.0 + f), z = sv * sv;
    const double R = z * (6.666666666666735130e-01 + z * (3.999999999940941908e-01 + z * (2.857142874366239149e-01 + z * (2.222219843214978396e-01 +
                     z * (1.818357216161805012e-01 + z * (1.531383769920937332e-01 + z * 1.479819860511658591e-01))))));
    const double kd = (double)k;
    const double y = kd * 6.93147180369123816490e-01 - ((hfsq - (sv * (hfsq + R) + (kd * 1.90821492927058770002e-10 + c))) - f);
    return u < INFINITY ? y : u;
}

CVX_HD double rho(const Loss &l, double s)
{
    if (l.cauchy) return l.d2 * log1p_pos(s * l.inv_d2);
    return s <= l.d2 ? s : 2.0 * l.delta * sqrt(s) - l.d2;
}

// (no division on the quadratic branch: s = 0 is safe)
CVX_HD double rho_prime(const Loss &l, double s)
{
    if (l.cauchy) return 1.0 / (1.0 + s * l.inv_d2);
    return s <= l.d2 ? 1.0 : l.delta / sqrt(s);
}

// a problem's correspondences with their weights, and where the per-record output of the problem goes (points, lines; null: not wanted)
struct WProb {
    Prob pb;
    const double *wp, *wl;
    double *ow_p, *ow_l;
};

// Record k with its weight.  kind 0 and w = 0: not live;  kind 0 and w = -1: admitted by its mask with a weight that is negative or not
// finite;  otherwise w > 0 and finite.  The weight is read only where the mask admits the record, the record only where the weight is usable.
CVX_HD void wrec_load(const WProb &wp, int k, Rec &r, double &w)
{
    const Prob &pb = wp.pb;
    double wk = 0.0;
    if (k < pb.n_p) {
        if (!pb.mp || pb.mp[k]) wk = wp.wp ? wp.wp[k] : 1.0;
    } else if (k < pb.n_p + pb.n_l) {
        if (!pb.ml || pb.ml[k - pb.n_p]) wk = wp.wl ? wp.wl[k - pb.n_p] : 1.0;
    }
    const bool usable = wk > 0.0 && wk < INFINITY;
    cvxr::rec_load(pb, usable ? k : pb.n_p + pb.n_l, r); // (beyond the last record: all zeros, nothing read)
    w = usable ? (r.kind != 0 ? wk : 0.0) : (wk == 0.0 ? 0.0 : -1.0);
}

// s_k of a live record at a pose: a light projection of both steps (no Jacobian); front: both depths positive
CVX_HD double rec_sq(const Rec &r, const Pose &ps, bool &front)
{
    double s = 0.0;
    front = true;
    CVX_ROLLED for (int st = 0; st < 2; ++st) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        cvxr::rec_step(r, st, X, alpha, beta, gamma);
        const bool f = cvxr::project(ps, X, yc, u, v, iw);
        const double res = alpha * u + beta * v + gamma;
        s += res * res;
        front = front && f;
    }
    return s;
}

// The sums of one record: both steps share omega = w rho'(s_k), so s_k is known before either step is accumulated -- by rec_sq, then
// refine_core.h's rolled loop with ONE copy of the projection and of the 27 accumulations.  (j omega first: with omega = 1 the products
// are those of cvxr::rec_acc.)  a[27], refine_core.h's cost, is not taken here: rho is evaluated at one site, wrec_cost.
CVX_HD void wrec_acc(const Rec &r, double w, const Pose &ps, const Loss &l, double *a)
{
    if (r.kind == 0) return;
    bool front;
    const double s = rec_sq(r, ps, front);
    const double om = w * rho_prime(l, s);
    CVX_ROLLED for (int st = 0; st < 2; ++st) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        cvxr::rec_step(r, st, X, alpha, beta, gamma);
        cvxr::project(ps, X, yc, u, v, iw);
        double j[6], q[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            q[i] = (alpha * (ps.K[i] - u * ps.K[6 + i]) + beta * (ps.K[3 + i] - v * ps.K[6 + i])) * iw;
        const double res = alpha * u + beta * v + gamma;
        cvxr::cross(yc, q, j);
        j[3] = q[0]; j[4] = q[1]; j[5] = q[2];
        int idx = 0;
        CVX_UNROLL for (int i = 0; i < 6; ++i) {
            const double jw = j[i] * om;
            CVX_UNROLL for (int k = i; k < 6; ++k) a[idx++] += jw * j[k];
            a[21 + i] += jw * res;
        }
    }
}

// robust cost of one record at a trial pose, infinite when a depth is not positive
CVX_HD void wrec_cost(const Rec &r, double w, const Pose &ps, const Loss &l, double *c1)
{
    if (r.kind == 0) return;
    bool front;
    const double s = rec_sq(r, ps, front);
    c1[0] += front ? w * rho(l, s) : INFINITY;
}

// centroid sums (UNWEIGHTED, as refine_core.h's) of the live records, and in s[5] the records with an unusable weight
CVX_HD void wrec_centre(const Rec &r, double w, double *s)
{
    cvxr::rec_centre(r, s);
    s[5] += w < 0.0 ? 1.0 : 0.0;
}

// refine_core.h's refine_problem on the robust cost.  LN is its lane interface with the weight and the index beside each record:
//   each(f)   f(const Rec &, double w, int64_t k) for every record this lane owns (records that are not live included);
//   sum<N>, any   as there.
// Same statuses, same schedule, same pass-through rules.  The cost before comes back in two ways and a caller uses ONE of them, the other
// is dead code after inlining: by value in cost_before, two vector registers that live through the loop (the scenes kernel and the host),
// or stored from inside the loop through cost_store, a pointer that only the writing lane holds (refine_core.h's way: the group kernels,
// whose vector registers are full where the scenes kernel's scalar ones are).
template <class LN>
CVX_HD void robust_problem(LN &ln, const double *Kp, const double *Rin, const double *tin, bool admit, const Opts &o, const Loss &l, Result &res,
                           double &cost_before, double *cost_store = nullptr)
{
    using namespace cvxr;
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
    ln.each([&](const Rec &r, double w, int64_t) { wrec_centre(r, w, s6); });
    ln.template sum<6>(s6);
    const int n_live = (int)s6[4];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s6[3] > 0.0 ? s6[i] / s6[3] : 0.0;
    double Rc[3];
    rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t0[i];

    int st = -1; // running
    if (!admit || !fin || !(det > 0.0)) st = REFINE_SKIPPED;
    else if (s6[5] > 0.0) st = REFINE_BEHIND; // a weight that is negative or not finite
    else if (n_live < 3) st = REFINE_SINGULAR;
    double acc[ACC_N];
    CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
    double cost = NAN, lambda = o.lambda0;
    cost_before = NAN;
    if (cost_store) *cost_store = NAN;
    int iters = 0;
    bool active = st < 0;
    int seen = 0; // bit 0 SOLVED, bit 1 MOVED (refine_core.h)

    // refine_core.h's loop turned by half an iteration, so that the robust cost is evaluated at ONE site (two copies of rho -- a square
    // root, a logarithm -- do not fit beside the loop's state): a pass begins with the cost of the pose in `tr` -- the input pose in pass
    // 0, afterwards the trial of the pass before, which is then judged -- and goes on to the sums and the step of the next trial.  The
    // trials, their order and what is decided of them are refine_core.h's.
    Pose tr = ps;
    bool ok = false;
    double rel = 0.0;
    for (int it = 0;; ++it) {
        double c1[1] = {0.0};
        ln.each([&](const Rec &r, double w, int64_t) { wrec_cost(r, w, tr, l, c1); });
        ln.template sum<1>(c1);
        if (it == 0) {
            if (active) {
                cost = c1[0];
                if (!(cost < INFINITY)) { st = REFINE_BEHIND; active = false; } // (a NaN or inf among the live records' numbers ends here too)
                else {
                    cost_before = cost;
                    if (cost_store) *cost_store = cost;
                }
            }
        } else if (active) {
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
                st = REFINE_CONVERGED; active = false;
            } else {
                lambda *= 10.0;
                if (lambda > LAMBDA_MAX) { st = (seen & 1) ? REFINE_MAXITER : REFINE_SINGULAR; active = false; }
            }
        }
        if (!(ln.any(active) && it < o.max_iters)) break; // no other trial follows
        // the ONE site that takes the sums: re-weighted at the pose each problem has reached
        CVX_UNROLL for (int i = 0; i < ACC_N; ++i) acc[i] = 0.0;
        ln.each([&](const Rec &r, double w, int64_t) { wrec_acc(r, w, ps, l, acc); });
        ln.template sum<ACC_N - 1>(acc);
        double d[6];
        ok = damped_step(acc, lambda, d);
        CVX_PHASE();
        rel = step_measure(ps, d);
        tr = ps;
        pose_step(tr, d);
        CVX_PHASE();
    }
    if (st < 0) st = REFINE_MAXITER;
    const bool done = st <= REFINE_MAXITER;
    if (!done) { // (lambda ran out before any system was positive definite)
        cost_before = NAN;
        if (cost_store) *cost_store = NAN;
    }
    rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 9; ++i) res.R[i] = ps.R[i];
    CVX_UNROLL for (int i = 0; i < 3; ++i) res.t[i] = (seen & 2) ? ps.tc[i] - Rc[i] : tin[i]; // (a pose no trial moved: t bit for bit)
    res.cost = done ? cost : NAN;
    res.iters = done ? iters : 0; res.status = st; res.n_live = n_live;
}

// What comes back per record, a pass of its own over the same lanes after robust_problem (kept out of its loop: the register file):
// rho'(s_k) at the returned pose (R, t) -- 0 for a record that is not live, NaN for every record of a problem that was not refined
// (status 2-4) -- and the number of live records with s_k <= delta^2 (0 for a problem that was not refined).  Every lane of the problem
// returns the count.  The chart's centre plays no part here: c = 0.
template <class LN>
CVX_HD int robust_weights_problem(LN &ln, const WProb &wp, const double *Kp, const double *R, const double *t, int status, const Loss &l)
{
    Pose ps;
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = R[i]; }
    CVX_UNROLL for (int i = 0; i < 3; ++i) { ps.c[i] = 0.0; ps.tc[i] = t[i]; }
    const bool done = status <= cvxr::REFINE_MAXITER;
    double cnt[1] = {0.0};
    ln.each([&](const Rec &r, double, int64_t k) {
        double rw = 0.0;
        if (r.kind != 0 && done) {
            bool front;
            const double s = rec_sq(r, ps, front);
            rw = rho_prime(l, s);
            cnt[0] += s <= l.d2 ? 1.0 : 0.0;
        }
        if (!done) rw = NAN;
        double *o = k < wp.pb.n_p ? wp.ow_p : wp.ow_l;
        const int64_t ko = k < wp.pb.n_p ? k : k - wp.pb.n_p;
        if (o && k < (int64_t)wp.pb.n_p + wp.pb.n_l) o[ko] = rw;
    });
    ln.template sum<1>(cnt);
    return (int)cnt[0];
}

// the host's lanes: one lane owns the whole problem
struct HostLanes {
    WProb wp;
    template <class F>
    void each(F f)
    {
        const int n = wp.pb.n_p + wp.pb.n_l;
        for (int k = 0; k < n; ++k) {
            Rec r;
            double w;
            wrec_load(wp, k, r, w);
            f(r, w, (int64_t)k);
        }
    }
    template <int N>
    void sum(double *) {}
    bool any(bool p) { return p; }
};

} // namespace cvxrb
