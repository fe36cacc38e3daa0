// refine_robust_sanitize_main.cpp -- a stand-alone program over cvxpnpl_refine_robust_batch_host, compiled FROM SOURCE together with
// cvxpnpl_amd/csrc/host_refine_robust.cpp under -fsanitize=address,undefined by tests/test_refine_robust_library.py: the shapes at which
// an index of the robust refinement can go wrong on the host -- no points, no lines, 65 records with masks and weights, a null robust_w, a
// strided status column, all three losses.  Guard words around every output show a write outside it even where the sanitizer's red zones
// would not.  Exit code 0 and "ok" on success; any sanitizer report aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_robust.h"

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
    T *p() { return n ? v.data() + 8 : nullptr; }
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

const double GUARD_D = -7.25e300; // (not NaN: robust_w of a problem that was not refined IS NaN)

int run(int64_t B, int n_p, int n_l, bool masks, bool weights, bool want_w, bool strided, int loss)
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
    std::vector<uint8_t> mp((size_t)B * n_p, 1), ml((size_t)B * n_l, 1);
    std::vector<double> wp((size_t)B * n_p), wl((size_t)B * n_l);
    for (double &w : wp) w = 0.1 + 1.9 * uni();
    for (double &w : wl) w = 0.1 + 1.9 * uni();
    if (masks) {
        for (size_t i = 2; i < mp.size(); i += 3) { mp[i] = 0; p2[2 * i] = NAN; p3[3 * i] = 1e9; wp[i] = NAN; }
        for (size_t i = 1; i < ml.size(); i += 3) { ml[i] = 0; l2[4 * i + 3] = NAN; l3[6 * i] = 1e9; wl[i] = -1.0; }
    }
    if (weights) { // a zero weight is a mask too: the spoiled record behind it is never read
        for (size_t i = 1; i < wp.size(); i += 3) { wp[i] = 0.0; p2[2 * i + 1] = NAN; p3[3 * i + 2] = 1e9; }
        for (size_t i = 2; i < wl.size(); i += 3) { wl[i] = 0.0; l2[4 * i] = NAN; l3[6 * i + 4] = 1e9; }
    }
    const int64_t stride = strided ? 3 : 1;
    std::vector<int32_t> status((size_t)B * stride, 7);
    for (int64_t b = 0; b < B; ++b) status[b * stride] = b % 5 == 4 ? 1 : 0; // every fifth problem: not admitted
    Guarded<double> oR((size_t)B * 9, GUARD_D), ot((size_t)B * 3, GUARD_D), cost((size_t)B * 2, GUARD_D), rw(want_w ? (size_t)B * n : 0, GUARD_D);
    Guarded<int32_t> iters((size_t)B, -77), ost((size_t)B, -77), n_live((size_t)B, -77), n_in((size_t)B, -77);
    cvxpnpl_refine_robust_opts_t o;
    o.struct_size = sizeof o; o.max_iters = 40; o.step_tol = 1e-10; o.lambda0 = 1e-3; o.loss = loss; o.scale_px = 0.4;
    const int rc = cvxpnpl_refine_robust_batch_host(B, n_p, n_p ? p2.data() : nullptr, n_p ? p3.data() : nullptr, n_l, n_l ? l2.data() : nullptr,
                                                    n_l ? l3.data() : nullptr, K, 0, R.data(), t.data(), status.data(), stride, 1u,
                                                    masks && n_p ? mp.data() : nullptr, masks && n_l ? ml.data() : nullptr,
                                                    (weights || masks) && n_p ? wp.data() : nullptr, (weights || masks) && n_l ? wl.data() : nullptr, &o, oR.p(),
                                                    ot.p(), cost.p(), iters.p(), ost.p(), n_live.p(), rw.p(), n_in.p(), 3);
    if (rc != 0) { printf("rc %d: %s\n", rc, cvxpnpl_refine_robust_last_error()); return 1; }
    if (!oR.intact() || !ot.intact() || !cost.intact() || !rw.intact() || !iters.intact() || !ost.intact() || !n_live.intact() || !n_in.intact()) {
        printf("a guard was overwritten\n");
        return 1;
    }
    if (!oR.written() || !ot.written() || !cost.written() || !rw.written() || !iters.written() || !ost.written() || !n_live.written() || !n_in.written()) {
        printf("an output element was left unwritten\n");
        return 1;
    }
    for (int64_t b = 0; b < B; ++b) {
        const int st = ost.p()[b];
        const bool skipped = b % 5 == 4;
        if (skipped ? st != 2 : (st != 0 && st != 1)) { printf("B=%lld n_p=%d n_l=%d loss %d: problem %lld status %d\n", (long long)B, n_p, n_l, loss, (long long)b, st); return 1; }
        if (n_in.p()[b] < 0 || n_in.p()[b] > n_live.p()[b] || n_live.p()[b] > n) { printf("counts out of range\n"); return 1; }
        if (want_w)
            for (int k = 0; k < n; ++k) {
                const double w = rw.p()[b * n + k];
                if (skipped ? !std::isnan(w) : !(w >= 0.0 && w <= 1.0)) { printf("robust_w[%lld][%d] = %g\n", (long long)b, k, w); return 1; }
            }
    }
    return 0;
}

} // namespace

int main()
{
    int bad = 0;
    for (int loss = 0; loss < 3; ++loss) {
        bad += run(7, 0, 9, true, false, true, false, loss);    // no points
        bad += run(7, 9, 0, true, false, true, true, loss);     // no lines, a strided status column
        bad += run(5, 40, 25, true, true, true, false, loss);   // 65 records with masks and weights
        bad += run(5, 40, 25, false, true, false, true, loss);  // a null robust_w
        bad += run(1, 6, 0, false, false, true, false, loss);   // no masks, no weights
    }
    if (cvxpnpl_refine_robust_batch_host(0, 3, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, 1u, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_refine_robust_batch_host(2, 3, nullptr, nullptr, 0, nullptr, nullptr, K, 0, K, K, nullptr, 1, 1u, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != -1) ++bad;
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
