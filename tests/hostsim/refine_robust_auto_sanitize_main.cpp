// refine_robust_auto_sanitize_main.cpp -- a stand-alone program over the host entry points of the twelfth library, compiled FROM SOURCE
// together with cvxpnpl_amd/csrc/host_refine_robust_auto.cpp under -fsanitize=address,undefined by tests/test_refine_robust_auto_library.py:
// the shapes at which an index of the scale estimate, of the loop at a scale per problem or of the covariance can go wrong on the host --
// ties (every record a copy of one), no points, no lines, problems with no live record at all, 65 records with masks and weights, bad
// scale elements, a strided status column, a zero batch.  Guard words around every output show a write outside it even where the
// sanitizer's red zones would not.  Exit code 0 and "ok" on success; any sanitizer report aborts.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_robust_auto.h"

namespace {

uint64_t state = 88172645463325252ULL;
double uni() // xorshift, in [0, 1)
{
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
}

const double K[9] = {800.0, 0.0, 320.0, 0.0, 800.0, 240.0, 0.0, 0.0, 1.0};

void pixel(const double *X, double *x)
{
    x[0] = K[0] * X[0] / X[2] + K[2] + (uni() - 0.5);
    x[1] = K[4] * X[1] / X[2] + K[5] + (uni() - 0.5);
}

template <class T>
struct Guarded { // n elements with 8 guard words on either side
    std::vector<T> v;
    size_t n;
    T guard;
    Guarded(size_t n_, T guard_) : v(n_ + 16, guard_), n(n_), guard(guard_) {}
    T *p() { return v.data() + 8; }
    bool same(T a) const { return std::memcmp(&a, &guard, sizeof(T)) == 0; }
    bool intact() const
    {
        for (size_t i = 0; i < 8; ++i)
            if (!same(v[i]) || !same(v[8 + n + i])) return false;
        return true;
    }
    bool written() const
    {
        for (size_t i = 0; i < n; ++i)
            if (same(v[8 + i])) return false;
        return true;
    }
};

const double GUARD_D = -7.25e300;

// mode 0: random records; 1: every record of a problem a copy of its first (ties); 2: every record masked (no live record)
int run(int64_t B, int n_p, int n_l, int mode, bool masks, bool weights, bool strided, int loss)
{
    const int n = n_p + n_l;
    std::vector<double> p2((size_t)B * n_p * 2), p3((size_t)B * n_p * 3), l2((size_t)B * n_l * 4), l3((size_t)B * n_l * 6), R((size_t)B * 9, 0.0), t((size_t)B * 3, 0.0);
    for (int64_t b = 0; b < B; ++b) R[9 * b] = R[9 * b + 4] = R[9 * b + 8] = 1.0;
    for (size_t i = 0; i < (size_t)B * n_p; ++i) {
        double *X = &p3[3 * i];
        X[0] = 2.0 * uni() - 1.0; X[1] = 2.0 * uni() - 1.0; X[2] = 4.0 + 4.0 * uni();
        pixel(X, &p2[2 * i]);
    }
    for (size_t i = 0; i < (size_t)B * n_l * 2; ++i) {
        double *X = &l3[3 * i];
        X[0] = 2.0 * uni() - 1.0; X[1] = 2.0 * uni() - 1.0; X[2] = 4.0 + 4.0 * uni();
        pixel(X, &l2[2 * i]);
    }
    if (mode == 1)
        for (int64_t b = 0; b < B; ++b) {
            for (int k = 1; k < n_p; ++k) { std::memcpy(&p2[(b * n_p + k) * 2], &p2[b * n_p * 2], 16); std::memcpy(&p3[(b * n_p + k) * 3], &p3[b * n_p * 3], 24); }
            for (int k = 1; k < n_l; ++k) { std::memcpy(&l2[(b * n_l + k) * 4], &l2[b * n_l * 4], 32); std::memcpy(&l3[(b * n_l + k) * 6], &l3[b * n_l * 6], 48); }
        }
    std::vector<uint8_t> mp((size_t)B * n_p, mode == 2 ? 0 : 1), ml((size_t)B * n_l, mode == 2 ? 0 : 1);
    std::vector<double> wp((size_t)B * n_p), wl((size_t)B * n_l);
    for (double &w : wp) w = 0.1 + 1.9 * uni();
    for (double &w : wl) w = 0.1 + 1.9 * uni();
    if (masks && mode == 0) {
        for (size_t i = 2; i < mp.size(); i += 3) { mp[i] = 0; p2[2 * i] = NAN; p3[3 * i] = 1e9; wp[i] = NAN; }
        for (size_t i = 1; i < ml.size(); i += 3) { ml[i] = 0; l2[4 * i + 3] = NAN; l3[6 * i] = 1e9; wl[i] = -1.0; }
    }
    if (weights && mode == 0) {
        for (size_t i = 1; i < wp.size(); i += 3) { wp[i] = 0.0; p2[2 * i + 1] = NAN; p3[3 * i + 2] = 1e9; }
        for (size_t i = 2; i < wl.size(); i += 3) { wl[i] = 0.0; l2[4 * i] = NAN; l3[6 * i + 4] = 1e9; }
    }
    const bool use_m = masks || mode == 2, use_w = weights || masks;
    const int64_t stride = strided ? 3 : 1;
    std::vector<int32_t> status((size_t)B * stride, 7);
    for (int64_t b = 0; b < B; ++b) status[b * stride] = b % 5 == 4 ? 1 : 0; // every fifth problem: not admitted
    const double *P2 = n_p ? p2.data() : nullptr, *P3 = n_p ? p3.data() : nullptr, *L2 = n_l ? l2.data() : nullptr, *L3 = n_l ? l3.data() : nullptr;
    const uint8_t *MP = use_m && n_p ? mp.data() : nullptr, *ML = use_m && n_l ? ml.data() : nullptr;
    const double *WP = use_w && n_p ? wp.data() : nullptr, *WL = use_w && n_l ? wl.data() : nullptr;

    // 1. the scale
    Guarded<double> sigma((size_t)B, GUARD_D), med((size_t)B, GUARD_D), sq((size_t)B * n, GUARD_D);
    Guarded<int32_t> n_live((size_t)B, -77), sst((size_t)B, -77);
    int rc = cvxpnpl_robust_scale_batch_host(B, n_p, P2, P3, n_l, L2, L3, K, 0, R.data(), t.data(), status.data(), stride, 1u, MP, ML, WP, WL, sigma.p(), med.p(),
                                             n_live.p(), sst.p(), sq.p(), 3);
    if (rc != 0) { printf("scale rc %d: %s\n", rc, cvxpnpl_refine_robust_auto_last_error()); return 1; }
    if (!sigma.intact() || !med.intact() || !sq.intact() || !n_live.intact() || !sst.intact()) { printf("scale: a guard was overwritten\n"); return 1; }
    if (!sigma.written() || !med.written() || !sq.written() || !n_live.written() || !sst.written()) { printf("scale: an output element was left unwritten\n"); return 1; }
    std::vector<double> scale((size_t)B);
    for (int64_t b = 0; b < B; ++b) {
        const int st = sst.p()[b], m = n_live.p()[b];
        const int want = b % 5 == 4 ? 2 : (m < 3 ? 3 : 0);
        if (st != want) { printf("scale: B=%lld n_p=%d n_l=%d mode %d problem %lld status %d, expected %d\n", (long long)B, n_p, n_l, mode, (long long)b, st, want); return 1; }
        std::vector<double> live;
        for (int k = 0; k < n; ++k) {
            const double s = sq.p()[b * n + k];
            if (st != 0 ? !std::isnan(s) : !(s == -1.0 || s >= 0.0)) { printf("sq[%lld][%d] = %g\n", (long long)b, k, s); return 1; }
            if (s >= 0.0) live.push_back(s);
        }
        if (st == 0) {
            if ((int)live.size() != m) { printf("scale: n_live %d, %zu values\n", m, live.size()); return 1; }
            std::sort(live.begin(), live.end());
            const double want_med = (m & 1) ? live[(m - 1) / 2] : 0.5 * (live[m / 2 - 1] + live[m / 2]);
            if (std::memcmp(&want_med, &med.p()[b], 8) != 0) { printf("scale: med_sq %.17g, the sorted values give %.17g\n", med.p()[b], want_med); return 1; }
            if (mode == 1 && n_l == 0 && want_med != live[0]) { printf("ties: the median is not the tied value\n"); return 1; }
        } else if (!std::isnan(sigma.p()[b]) || !std::isnan(med.p()[b])) { printf("scale: a number for status %d\n", st); return 1; }
        scale[b] = std::max(2.4477468306808166 * sigma.p()[b], 1e-3);
        if (b % 7 == 3) scale[b] = b % 2 ? 0.0 : NAN; // bad scale elements
    }

    // 2. the loop at a scale per problem
    Guarded<double> oR((size_t)B * 9, GUARD_D), ot((size_t)B * 3, GUARD_D), cost((size_t)B * 2, GUARD_D), rw((size_t)B * n, GUARD_D);
    Guarded<int32_t> iters((size_t)B, -77), ost((size_t)B, -77), nl2((size_t)B, -77), n_in((size_t)B, -77);
    cvxpnpl_refine_robust_opts_t o;
    o.struct_size = sizeof o; o.max_iters = 40; o.step_tol = 1e-10; o.lambda0 = 1e-3; o.loss = loss; o.scale_px = 0.4;
    rc = cvxpnpl_refine_robust_pp_batch_host(B, n_p, P2, P3, n_l, L2, L3, K, 0, R.data(), t.data(), status.data(), stride, 1u, MP, ML, WP, WL, scale.data(), &o, oR.p(),
                                             ot.p(), cost.p(), iters.p(), ost.p(), nl2.p(), rw.p(), n_in.p(), 3);
    if (rc != 0) { printf("loop rc %d: %s\n", rc, cvxpnpl_refine_robust_auto_last_error()); return 1; }
    if (!oR.intact() || !ot.intact() || !cost.intact() || !rw.intact() || !iters.intact() || !ost.intact() || !nl2.intact() || !n_in.intact()) {
        printf("loop: a guard was overwritten\n");
        return 1;
    }
    if (!oR.written() || !ot.written() || !cost.written() || !rw.written() || !iters.written() || !ost.written() || !nl2.written() || !n_in.written()) {
        printf("loop: an output element was left unwritten\n");
        return 1;
    }
    for (int64_t b = 0; b < B; ++b) {
        const int st = ost.p()[b], s0 = sst.p()[b];
        const bool bad_scale = loss != 0 && !(scale[b] > 0.0 && scale[b] < INFINITY);
        const bool fine = mode == 1 ? st <= 3 : st <= 1; // (copies of one record: the normal equations may be singular)
        if (s0 == 2 ? st != 2 : (bad_scale ? st != 4 : (s0 == 3 ? st != 3 : !fine))) {
            printf("loop: B=%lld n_p=%d n_l=%d mode %d loss %d problem %lld status %d (scale status %d, scale %g)\n", (long long)B, n_p, n_l, mode, loss, (long long)b, st, s0, scale[b]);
            return 1;
        }
        if (st > 1 && (std::memcmp(oR.p() + 9 * b, R.data() + 9 * b, 72) != 0 || std::memcmp(ot.p() + 3 * b, t.data() + 3 * b, 24) != 0)) { printf("loop: a pose did not pass through\n"); return 1; }
    }

    // 3. the covariance at the poses reached
    Guarded<double> cov((size_t)B * 36, GUARD_D);
    Guarded<int32_t> cst((size_t)B, -77);
    rc = cvxpnpl_robust_cov_batch_host(B, n_p, P2, P3, n_l, L2, L3, K, 0, oR.p(), ot.p(), ost.p(), MP, ML, WP, WL, loss, 1.0, scale.data(), cov.p(), cst.p(), 3);
    if (rc != 0) { printf("cov rc %d: %s\n", rc, cvxpnpl_refine_robust_auto_last_error()); return 1; }
    if (!cov.intact() || !cst.intact() || !cov.written() || !cst.written()) { printf("cov: a guard was overwritten or an element left unwritten\n"); return 1; }
    for (int64_t b = 0; b < B; ++b) {
        const int st = cst.p()[b];
        if (ost.p()[b] > 1 ? st != 2 : (st != 0 && st != 3)) { printf("cov: problem %lld status %d after loop status %d\n", (long long)b, st, ost.p()[b]); return 1; }
        for (int i = 0; i < 36; ++i)
            if ((st == 0) != std::isfinite(cov.p()[36 * b + i])) { printf("cov: status %d and cov[%d] = %g\n", st, i, cov.p()[36 * b + i]); return 1; }
    }
    return 0;
}

} // namespace

int main()
{
    int bad = 0;
    for (int loss = 0; loss < 3; ++loss) {
        for (int m = 3; m <= 6; ++m) bad += run(3, m, 0, 1, false, false, false, loss); // ties: m copies of one point
        bad += run(3, 0, 4, 1, false, false, false, loss);   // ... of one line
        bad += run(7, 0, 9, 0, true, false, false, loss);    // no points
        bad += run(7, 9, 0, 0, true, false, true, loss);     // no lines, a strided status column
        bad += run(8, 40, 25, 0, true, true, false, loss);   // 65 records with masks and weights, bad scale elements
        bad += run(8, 40, 25, 0, false, true, true, loss);
        bad += run(6, 5, 4, 2, false, false, false, loss);   // no live record
        bad += run(1, 6, 0, 0, false, false, false, loss);   // no masks, no weights
    }
    const double *z = nullptr;
    if (cvxpnpl_robust_scale_batch_host(0, 3, z, z, 0, z, z, z, 0, z, z, nullptr, 1, 1u, nullptr, nullptr, z, z, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_refine_robust_pp_batch_host(0, 3, z, z, 0, z, z, z, 0, z, z, nullptr, 1, 1u, nullptr, nullptr, z, z, z, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_robust_cov_batch_host(0, 3, z, z, 0, z, z, z, 0, z, z, nullptr, nullptr, nullptr, z, z, 1, 1.0, z, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_robust_scale_batch_host(2, 3, z, z, 0, z, z, K, 0, K, K, nullptr, 1, 1u, nullptr, nullptr, z, z, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != -1) ++bad;
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
