// refine_vjp_sanitize_main.cpp -- a stand-alone program over cvxpnpl_refine_vjp_batch_host, compiled FROM SOURCE together with
// cvxpnpl_amd/csrc/host_refine_vjp.cpp under -fsanitize=address,undefined by tests/test_refine_grad_library.py: the shapes at which an
// index of the backward pass can go wrong on the host -- no points, no lines, 65 records with masks, null gradient pointers, a strided
// status column.  Guard bytes of NaN around every output show a write outside it even where the sanitizer's red zones would not.
// Exit code 0 and "ok" on success; any sanitizer report aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cvxpnpl_amd_refine_grad.h"

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

struct Guarded { // n doubles with 8 NaN on either side
    std::vector<double> v;
    size_t n;
    explicit Guarded(size_t n_) : v(n_ + 16, NAN), n(n_) {}
    double *p() { return n ? v.data() + 8 : nullptr; }
    bool intact() const
    {
        for (size_t i = 0; i < 8; ++i)
            if (!std::isnan(v[i]) || !std::isnan(v[8 + n + i])) return false;
        return true;
    }
    bool written() const
    {
        for (size_t i = 0; i < n; ++i)
            if (std::isnan(v[8 + i])) return false;
        return true;
    }
};

int run(int64_t B, int n_p, int n_l, bool masks, bool want2, bool want3, bool strided)
{
    std::vector<double> p2((size_t)B * n_p * 2), p3((size_t)B * n_p * 3), l2((size_t)B * n_l * 4), l3((size_t)B * n_l * 6), R((size_t)B * 9, 0.0), t((size_t)B * 3, 0.0);
    std::vector<double> gR((size_t)B * 9), gt((size_t)B * 3);
    for (int64_t b = 0; b < B; ++b) {
        R[9 * b] = R[9 * b + 4] = R[9 * b + 8] = 1.0;
        for (int i = 0; i < 9; ++i) gR[9 * b + i] = uni() - 0.5;
        for (int i = 0; i < 3; ++i) gt[3 * b + i] = uni() - 0.5;
    }
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
    for (size_t i = 2; i < mp.size(); i += 3) { mp[i] = 0; p2[2 * i] = NAN; p3[3 * i] = 1e9; }
    for (size_t i = 1; i < ml.size(); i += 3) { ml[i] = 0; l2[4 * i + 3] = NAN; l3[6 * i] = 1e9; }
    const int64_t stride = strided ? 3 : 1;
    std::vector<int32_t> status((size_t)B * stride, 7);
    for (int64_t b = 0; b < B; ++b) status[b * stride] = b % 5 == 4 ? 1 : 0;
    Guarded g2(want2 ? (size_t)B * n_p * 2 : 0), g3(want3 ? (size_t)B * n_p * 3 : 0), h2(want2 ? (size_t)B * n_l * 4 : 0), h3(want3 ? (size_t)B * n_l * 6 : 0),
        info((size_t)B * 2);
    std::vector<int32_t> vst((size_t)B + 2, -7);
    const int rc = cvxpnpl_refine_vjp_batch_host(B, n_p, n_p ? p2.data() : nullptr, n_p ? p3.data() : nullptr, n_l, n_l ? l2.data() : nullptr,
                                                 n_l ? l3.data() : nullptr, K, 0, R.data(), t.data(), status.data(), stride, 1u,
                                                 masks && n_p ? mp.data() : nullptr, masks && n_l ? ml.data() : nullptr, gR.data(), want3 ? gt.data() : nullptr,
                                                 g2.p(), g3.p(), h2.p(), h3.p(), vst.data() + 1, info.p(), 3);
    if (rc != 0) { printf("rc %d: %s\n", rc, cvxpnpl_refine_grad_last_error()); return 1; }

    if (vst[0] != -7 || vst[B + 1] != -7) { printf("vjp_status written out of bounds\n"); return 1; }
    for (int64_t b = 0; b < B; ++b) {
        const int want = b % 5 == 4 ? 1 : 0;
        if (vst[b + 1] != want) { printf("B=%lld n_p=%d n_l=%d: problem %lld status %d, expected %d\n", (long long)B, n_p, n_l, (long long)b, vst[b + 1], want); return 1; }
    }
    Guarded *all[5] = {&g2, &g3, &h2, &h3, &info};
    for (Guarded *g : all) {
        if (!g->intact()) { printf("a guard was overwritten\n"); return 1; }
        if (g != &info && !g->written()) { printf("an output element was left unwritten\n"); return 1; }
    }
    return 0;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run(7, 0, 9, true, true, true, false);   // no points
    bad += run(7, 9, 0, true, true, true, true);    // no lines, a strided status column
    bad += run(5, 40, 25, true, true, true, false); // 65 records with masks
    bad += run(5, 40, 25, true, false, true, true); // null 2D gradient pointers
    bad += run(5, 40, 25, true, true, false, false); // null 3D gradient pointers and a null grad_t
    bad += run(1, 6, 0, true, false, false, false); // nothing wanted but the status
    if (cvxpnpl_refine_vjp_batch_host(0, 3, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, 1u, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != 0) ++bad;
    if (cvxpnpl_refine_vjp_batch_host(2, 3, nullptr, nullptr, 0, nullptr, nullptr, K, 0, K, K, nullptr, 1, 1u, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != -1) ++bad;
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
