// refine_robust_vjp_sanitize_main.cpp -- a stand-alone program over cvxpnpl_refine_robust_vjp_batch_host, compiled FROM SOURCE together
// with cvxpnpl_amd/csrc/host_refine_robust_vjp.cpp under -fsanitize=address,undefined by tests/test_refine_robust_grad_library.py: the
// shapes at which an index of the robust backward pass can go wrong on the host -- no points, no lines, 65 records with masks and
// weights, null gradient and weight-gradient pointers, a strided status column, all three losses.  Guard words around every output show
// a write outside it even where the sanitizer's red zones would not.  Exit code 0 and "ok" on success; any sanitizer report aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_robust_grad.h"

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

struct Guarded { // n doubles with 8 guard words on either side; the guard is a NaN with a payload of its own: no gradient is NaN
    std::vector<double> v;
    size_t n;
    double guard;
    explicit Guarded(size_t n_) : n(n_)
    {
        const uint64_t bits = 0x7ff8dead0000beefULL;
        std::memcpy(&guard, &bits, 8);
        v.assign(n + 16, guard);
    }
    double *p() { return n ? v.data() + 8 : nullptr; }
    bool same(double a) const { return std::memcmp(&a, &guard, 8) == 0; }
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
    bool finite() const
    {
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(v[8 + i])) return false;
        return true;
    }
};

// want: which of the six gradients are asked for (bit k: pts_2d, pts_3d, line_2d, line_3d, w_pts, w_lines)
int run(int64_t B, int n_p, int n_l, bool masks, bool weights, int want, bool strided, int loss)
{
    std::vector<double> p2((size_t)B * n_p * 2), p3((size_t)B * n_p * 3), l2((size_t)B * n_l * 4), l3((size_t)B * n_l * 6), R((size_t)B * 9, 0.0), t((size_t)B * 3, 0.0);
    std::vector<double> gR((size_t)B * 9), gt((size_t)B * 3);
    for (double &x : gR) x = uni() - 0.5;
    for (double &x : gt) x = uni() - 0.5;
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
    for (double &w : wp) w = 0.25 + 3.75 * uni();
    for (double &w : wl) w = 0.25 + 3.75 * uni();
    if (masks) { // behind a zero mask byte nothing is read: neither the spoiled record nor its weight
        for (size_t i = 2; i < mp.size(); i += 3) { mp[i] = 0; p2[2 * i] = NAN; p3[3 * i] = 1e9; wp[i] = NAN; }
        for (size_t i = 1; i < ml.size(); i += 3) { ml[i] = 0; l2[4 * i + 3] = NAN; l3[6 * i] = 1e9; wl[i] = -1.0; }
    }
    if (weights) { // a zero weight is a mask too
        for (size_t i = 1; i < wp.size(); i += 3) { wp[i] = 0.0; p2[2 * i + 1] = NAN; p3[3 * i + 2] = 1e9; }
        for (size_t i = 2; i < wl.size(); i += 3) { wl[i] = 0.0; l2[4 * i] = NAN; l3[6 * i + 4] = 1e9; }
    }
    const int64_t stride = strided ? 3 : 1;
    std::vector<int32_t> status((size_t)B * stride, 7);
    for (int64_t b = 0; b < B; ++b) status[b * stride] = b % 5 == 4 ? 1 : 0; // every fifth problem: not admitted
    Guarded g2(want & 1 ? (size_t)B * n_p * 2 : 0), g3(want & 2 ? (size_t)B * n_p * 3 : 0), h2(want & 4 ? (size_t)B * n_l * 4 : 0),
        h3(want & 8 ? (size_t)B * n_l * 6 : 0), gwp(want & 16 ? (size_t)B * n_p : 0), gwl(want & 32 ? (size_t)B * n_l : 0), info((size_t)B * 2);
    std::vector<int32_t> vst((size_t)B + 16, -77);
    const bool use_w = weights || masks;
    const int rc = cvxpnpl_refine_robust_vjp_batch_host(B, n_p, n_p ? p2.data() : nullptr, n_p ? p3.data() : nullptr, n_l, n_l ? l2.data() : nullptr,
                                                        n_l ? l3.data() : nullptr, K, 0, R.data(), t.data(), status.data(), stride, 1u, loss, 0.6,
                                                        masks && n_p ? mp.data() : nullptr, masks && n_l ? ml.data() : nullptr,
                                                        use_w && n_p ? wp.data() : nullptr, use_w && n_l ? wl.data() : nullptr, gR.data(), gt.data(),
                                                        g2.p(), g3.p(), h2.p(), h3.p(), gwp.p(), gwl.p(), vst.data() + 8, info.p(), 3);
    if (rc != 0) { printf("rc %d: %s\n", rc, cvxpnpl_refine_robust_grad_last_error()); return 1; }
    Guarded *all[7] = {&g2, &g3, &h2, &h3, &gwp, &gwl, &info};
    for (int i = 0; i < 7; ++i) {
        if (!all[i]->intact()) { printf("a guard of output %d was overwritten\n", i); return 1; }
        if (!all[i]->written()) { printf("an element of output %d was left unwritten\n", i); return 1; }
        if (i < 6 && !all[i]->finite()) { printf("output %d holds a number that is not finite\n", i); return 1; }
    }
    for (int i = 0; i < 8; ++i)
        if (vst[i] != -77 || vst[8 + B + i] != -77) { printf("a guard of vjp_status was overwritten\n"); return 1; }
    for (int64_t b = 0; b < B; ++b) {
        const int st = vst[8 + b];
        if (st != (b % 5 == 4 ? 1 : 0)) { printf("B=%lld n_p=%d n_l=%d loss %d: problem %lld vjp_status %d\n", (long long)B, n_p, n_l, loss, (long long)b, st); return 1; }
    }
    // records that are not live: exact zeros, their weights' gradients too
    if (weights && (want & 16))
        for (size_t i = 1; i < wp.size(); i += 3)
            if (gwp.p()[i] != 0.0) { printf("a zero weight has a gradient\n"); return 1; }
    if (masks && (want & 8))
        for (size_t i = 1; i < ml.size(); i += 3)
            for (int c = 0; c < 6; ++c)
                if (h3.p()[6 * i + c] != 0.0) { printf("a masked line has a gradient\n"); return 1; }
    return 0;
}

} // namespace

int main()
{
    int bad = 0;
    for (int loss = 0; loss < 3; ++loss) {
        bad += run(7, 0, 9, true, false, 63, false, loss);    // no points
        bad += run(7, 9, 0, true, false, 63, true, loss);     // no lines, a strided status column
        bad += run(5, 40, 25, true, true, 63, false, loss);   // 65 records with masks and weights
        bad += run(5, 40, 25, false, true, 16 + 32, true, loss); // the weights' gradients alone: four null gradient pointers
        bad += run(5, 40, 25, true, true, 1 + 8, false, loss);   // null weight-gradient pointers
        bad += run(1, 6, 0, false, false, 63, false, loss);   // no masks, no weights: the weights' gradients at w = 1
    }
    if (cvxpnpl_refine_robust_vjp_batch_host(0, 3, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 7, nullptr, nullptr, nullptr, 1, 1u, 9, NAN, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_refine_robust_vjp_batch_host(2, 3, nullptr, nullptr, 0, nullptr, nullptr, K, 0, K, K, nullptr, 1, 1u, 1, 1.0, nullptr, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != -1) ++bad;
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
