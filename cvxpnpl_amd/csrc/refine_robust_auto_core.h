// refine_robust_auto_core.h -- what the robust refinement lacks when every problem of a launch has a noise level of its own, host and
// device from one source.  Included, not edited: refine_core.h (records, the projection, the chart, the Cholesky),
// refine_robust_core.h (the loss, a record's weight, s_k, the loop, the lane interface with the weight and the index beside each record)
// and refine_robust_vjp_core.h (rho'' and the full Hessian).  Three things:
//
//   1. scale_problem       sigma of a problem from the MEDIAN of the s_k of its live records at a pose.  A point's s_k and a line's are both
//      chi^2_2 sigma^2 under isotropic Gaussian noise of sigma pixels per residual, whose median is 2 ln 2 sigma^2:
//          sigma = sqrt(med_sq / (2 ln 2)),   med_sq = numpy.median of the live s_k.
//      The median is UNWEIGHTED (a weight only decides whether a record is live).  It is found exactly and without sorting or atomics:
//      finite non-negative doubles order as their 64-bit patterns, so the order statistic of rank r is built bit by bit from the top -- for
//      bit b, the candidate is the prefix found so far with bit b set, and the bit stays iff at most r live values are below the candidate.
//      63 rounds of one count each (two for an even number of live records: both middle ranks walk together), the counts summed by the
//      lanes' existing exchange (exact in f64).  What is selected is an element of sq, bit for bit.
//   2. PerProblemScale     the lanes of robust_problem with the one hook a per-problem scale needs: an element that is not finite and > 0
//      cannot be rejected by the host without a synchronisation, so it is counted where a bad weight is (status 4, the pose passes through).
//   3. robust_cov_problem  the sandwich covariance of an M-estimate,  V_c = m / (m - 6) H^-1 B H^-1,  m = 2 n_live,
//          H = refine_robust_vjp_core.h's full Hessian (wrec_acc_full: residual curvature and the 2 w rho'' v v^T term),
//          B = sum_k omega_k^2 v_k v_k^T,   v_k = sum_i J_i r_i,   omega_k = w_k rho'(s_k),
//      in the centred chart, brought to the public chart by refine_core.h's M:  cov = M V_c M^T.  H in one pass over the records, its Cholesky,
//      then B in a second pass (42 + 7 accumulators beside the factor do not fit the register file), then per column two solves.
#pragma once
#include <string.h>

#include "refine_core.h"
#include "refine_robust_core.h"
#include "refine_robust_vjp_core.h"

namespace cvxra {

using cvxr::Pose;
using cvxr::Rec;
using cvxrb::Loss;
using cvxrb::WProb;

constexpr double CHI2_2_MEDIAN = 1.3862943611198906; // 2 ln 2

enum CovStatus : int { COV_OK = 0, COV_SKIPPED = 2, COV_SINGULAR = 3, COV_BEHIND = 4 };

CVX_HD uint64_t bits_of(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

CVX_HD double double_of(uint64_t u)
{
    double x;
    memcpy(&x, &u, 8);
    return x;
}

// a per-problem scale element that the loss can use (l2 does not look at it)
CVX_HD bool scale_usable(int loss_kind, double scale) { return loss_kind == cvxrb::LOSS_L2 || (scale > 0.0 && scale < INFINITY); }

struct ScaleResult {
    double sigma, med_sq;
    int n_live, status;
};

// The scale of one problem.  SL spreads the problem's records AND their s_k over the lanes:
//   first(f)     f(const Rec &, double w) -> double for every record this lane owns; the lane keeps what f returns as the record's value
//                (in a register, or in sq);
//   vals(f)      f(double) for every value this lane keeps;
//   finish(ok)   the values go to sq as they are (ok) or as NaN;
//   sum<N>       as refine_core.h's.
// The entry checks are robust_problem's, in its order.  The chart's centre plays no part in s_k: c = 0 (robust_weights_problem's choice).
// Every lane of the problem returns the same result.
template <class SL>
CVX_HD void scale_problem(SL &sl, const double *Kp, const double *Rin, const double *tin, bool admit, ScaleResult &res)
{
    Pose ps;
    CVX_UNROLL for (int i = 0; i < 9; ++i) { ps.K[i] = Kp[i]; ps.R[i] = Rin[i]; }
    CVX_UNROLL for (int i = 0; i < 3; ++i) { ps.c[i] = 0.0; ps.tc[i] = tin[i]; }
    bool fin = true;
    CVX_UNROLL for (int i = 0; i < 9; ++i) fin = fin && cvxr::finite(ps.R[i]);
    CVX_UNROLL for (int i = 0; i < 3; ++i) fin = fin && cvxr::finite(ps.tc[i]);
    const double det = ps.R[0] * (ps.R[4] * ps.R[8] - ps.R[5] * ps.R[7]) - ps.R[1] * (ps.R[3] * ps.R[8] - ps.R[5] * ps.R[6]) +
                       ps.R[2] * (ps.R[3] * ps.R[7] - ps.R[4] * ps.R[6]);
    double c3[3] = {0.0, 0.0, 0.0}; // live records, unusable weights, live records behind the camera or with a non-finite s
    sl.first([&](const Rec &r, double w) {
        c3[1] += w < 0.0 ? 1.0 : 0.0;
        if (r.kind == 0) return -1.0;
        bool front;
        const double s = cvxrb::rec_sq(r, ps, front);
        c3[0] += 1.0;
        c3[2] += front && s < INFINITY ? 0.0 : 1.0;
        return s;
    });
    sl.template sum<3>(c3);
    const int m = (int)c3[0];
    int st = 0;
    if (!admit || !fin || !(det > 0.0)) st = cvxr::REFINE_SKIPPED;
    else if (c3[1] > 0.0) st = cvxr::REFINE_BEHIND;
    else if (m < 3) st = cvxr::REFINE_SINGULAR;
    else if (c3[2] > 0.0) st = cvxr::REFINE_BEHIND;
    // the two middle ranks (the same rank twice for an odd m), walked together; every lane walks, whatever its problem's status: the
    // exchanges stay convergent
    const double r_lo = (double)((m - 1) / 2), r_hi = (double)(m / 2);
    uint64_t p_lo = 0, p_hi = 0;
    CVX_ROLLED for (int b = 62; b >= 0; --b) {
        const uint64_t c_lo = p_lo | (1ULL << b), c_hi = p_hi | (1ULL << b);
        double n2[2] = {0.0, 0.0};
        sl.vals([&](double s) {
            const uint64_t u = bits_of(s);
            const bool live = s >= 0.0;
            n2[0] += live && u < c_lo ? 1.0 : 0.0;
            n2[1] += live && u < c_hi ? 1.0 : 0.0;
        });
        sl.template sum<2>(n2);
        p_lo = n2[0] <= r_lo ? c_lo : p_lo;
        p_hi = n2[1] <= r_hi ? c_hi : p_hi;
    }
    const bool ok = st == 0;
    sl.finish(ok);
    const double med = (m & 1) ? double_of(p_lo) : 0.5 * (double_of(p_lo) + double_of(p_hi));
    res.med_sq = ok ? med : NAN;
    res.sigma = ok ? sqrt(med / CHI2_2_MEDIAN) : NAN;
    res.n_live = m;
    res.status = st;
}

// robust_problem's lanes (LN: refine_robust_core.h's lane interface) with a per-problem scale: where the scale element cannot be used,
// the count of unusable weights -- the sixth of the centre sums, the only sum<6> robust_problem takes -- is raised by one, so that the
// problem ends with status 4 at the place where a bad weight ends it, after the causes of status 2 and before the count of live records.
// This rests on robust_problem taking exactly ONE six-wide sum (refine_robust_core.h is included here, not edited, and cannot say so
// itself): tests/test_refine_robust_auto_host.py pins that, and fails if a second sum<6> appears or the centre sums change their width.
template <class LN>
struct PerProblemScale : LN {
    bool bad_scale;
    template <int N>
    CVX_HDM void sum(double *v)
    {
        LN::template sum<N>(v);
        if (N == 6 && bad_scale) v[5] += 1.0;
    }
};

// the outer products of one record's omega_k v_k: a[0, 21) += (omega v)(omega v)^T, upper triangle row by row
CVX_HD void wrec_meat(const Rec &r, double w, const Pose &ps, const Loss &l, double *a)
{
    if (r.kind == 0) return;
    bool front;
    const double sk = cvxrb::rec_sq(r, ps, front);
    const double om = w * cvxrb::rho_prime(l, sk);
    double gk[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    CVX_ROLLED for (int s = 0; s < 2; ++s) {
        double X[3], alpha, beta, gamma, yc[3], u, v, iw;
        cvxr::rec_step(r, s, X, alpha, beta, gamma);
        cvxr::project(ps, X, yc, u, v, iw);
        double j[6], q[3];
        CVX_UNROLL for (int i = 0; i < 3; ++i)
            q[i] = (alpha * (ps.K[i] - u * ps.K[6 + i]) + beta * (ps.K[3 + i] - v * ps.K[6 + i])) * iw;
        const double res = alpha * u + beta * v + gamma;
        cvxr::cross(yc, q, j);
        j[3] = q[0]; j[4] = q[1]; j[5] = q[2];
        CVX_UNROLL for (int i = 0; i < 6; ++i) gk[i] += j[i] * res;
    }
    int idx = 0;
    CVX_UNROLL for (int i = 0; i < 6; ++i) {
        const double gi = om * gk[i];
        CVX_UNROLL for (int c = i; c < 6; ++c) a[idx++] += gi * (om * gk[c]);
    }
}

// The sandwich covariance of one problem at (R, t) over refine_robust_core.h's lanes.  differentiated: the refinement's status was 0 or 1
// and the scale element is usable (the caller decides; false gives status 2 / 4 through `bad_scale`).  cov [36] (null on the lanes that
// do not write) is NaN unless the returned status is COV_OK.  Every lane of the problem returns the same status.
template <class LN>
CVX_HD int robust_cov_problem(LN &ln, const double *Kp, const double *Rin, const double *tin, bool differentiated, bool bad_scale, const Loss &l, double *cov)
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
    double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const Rec &r, double w, int64_t) { cvxrb::wrec_centre(r, w, s6); });
    ln.template sum<6>(s6);
    const int n_live = (int)s6[4];
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.c[i] = s6[3] > 0.0 ? s6[i] / s6[3] : 0.0;
    double Rc[3];
    cvxr::rot_c(ps, Rc);
    CVX_UNROLL for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t0[i];

    // first pass: H (and g, and the sum that is infinite when a live record is behind the camera)
    double acc[cvxrbg::ACC_N];
    CVX_UNROLL for (int i = 0; i < cvxrbg::ACC_N; ++i) acc[i] = 0.0;
    ln.each([&](const Rec &r, double w, int64_t) { cvxrbg::wrec_acc_full(r, w, ps, l, acc); });
    ln.template sum<cvxrbg::ACC_N>(acc);
    CVX_PHASE();
    int st = COV_OK;
    if (!differentiated || !fin || !(det > 0.0)) st = COV_SKIPPED;
    else if (s6[5] > 0.0 || bad_scale) st = COV_BEHIND;
    else if (n_live <= 3) st = COV_SINGULAR; // m <= 6: no degrees of freedom left
    else if (!(acc[27] < INFINITY)) st = COV_BEHIND;
    double Lm[36];
    {
        double A[36];
        CVX_UNROLL for (int i = 0; i < 6; ++i)
            CVX_UNROLL for (int c = 0; c < 6; ++c) A[i * 6 + c] = acc[cvxr::uidx(i, c)];
        const bool pd = cvxr::chol6(A, Lm);
        if (st == COV_OK && !pd) st = COV_SINGULAR; // the pose is not a strict minimum of the robust cost
    }
    CVX_PHASE();

    // second pass: B
    double Bm[21];
    CVX_UNROLL for (int i = 0; i < 21; ++i) Bm[i] = 0.0;
    ln.each([&](const Rec &r, double w, int64_t) { wrec_meat(r, w, ps, l, Bm); });
    ln.template sum<21>(Bm);
    CVX_PHASE();

    const double m = 2.0 * (double)n_live, f = m / (m - 6.0);
    const bool ok = st == COV_OK;
    const double S[9] = {0.0, -Rc[2], Rc[1], Rc[2], 0.0, -Rc[0], -Rc[1], Rc[0], 0.0};
    // column k of M H^-1 B H^-1 M^T: y = H^-1 (row k of M), z = B y, x = H^-1 z, then M x (refine_core.h's covariance(), applied twice)
    CVX_UNROLL for (int k = 0; k < 6; ++k) {
        double mk[6], y[6], z[6], x[6];
        CVX_UNROLL for (int i = 0; i < 6; ++i) mk[i] = i == k ? 1.0 : 0.0;
        if (k >= 3) CVX_UNROLL for (int i = 0; i < 3; ++i) mk[i] = S[3 * (k - 3) + i];
        cvxr::chol6_solve(Lm, mk, y);
        CVX_UNROLL for (int i = 0; i < 6; ++i) {
            double zi = 0.0;
            CVX_UNROLL for (int c = 0; c < 6; ++c) zi += Bm[cvxr::uidx(i, c)] * y[c];
            z[i] = zi;
        }
        cvxr::chol6_solve(Lm, z, x);
        if (cov) {
            CVX_UNROLL for (int i = 0; i < 3; ++i) {
                cov[i * 6 + k] = ok ? f * x[i] : NAN;
                cov[(3 + i) * 6 + k] = ok ? f * (S[3 * i] * x[0] + S[3 * i + 1] * x[1] + S[3 * i + 2] * x[2] + x[3 + i]) : NAN;
            }
        }
        CVX_PHASE();
    }
    return st;
}

// ---- the host's lanes: one lane owns the whole problem ----

// the values live in sq: points then lines (sq_l = sq_p + n_p in the batch form)
struct HostScaleLanes {
    WProb wp; // ow_p / ow_l: sq of the problem's points / lines
    double &at(int k) { return k < wp.pb.n_p ? wp.ow_p[k] : wp.ow_l[k - wp.pb.n_p]; }
    template <class F>
    void first(F f)
    {
        const int n = wp.pb.n_p + wp.pb.n_l;
        for (int k = 0; k < n; ++k) {
            Rec r;
            double w;
            cvxrb::wrec_load(wp, k, r, w);
            at(k) = f(r, w);
        }
    }
    template <class F>
    void vals(F f)
    {
        const int n = wp.pb.n_p + wp.pb.n_l;
        for (int k = 0; k < n; ++k) f(at(k));
    }
    void finish(bool ok)
    {
        const int n = wp.pb.n_p + wp.pb.n_l;
        if (!ok) for (int k = 0; k < n; ++k) at(k) = NAN;
    }
    template <int N>
    void sum(double *) {}
};

} // namespace cvxra
