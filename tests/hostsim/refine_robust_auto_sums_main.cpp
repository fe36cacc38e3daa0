// refine_robust_auto_sums_main.cpp -- a stand-alone program that prints the two halves of the sandwich covariance as the library's own
// source takes them: the 21 sums of H (cvxrbg::wrec_acc_full) and the 21 sums of B (cvxra::wrec_meat) over cvxrb::HostLanes, in the chart
// about the mean of the live 3D records, with that mean.  The C ABI returns only their product; tests/test_refine_robust_auto_host.py
// compiles this from source, brings both to the public chart and holds each against the difference reference on its own, so that an
// error which cancels in H^-1 B H^-1 cannot pass.  Input (text, on stdin): loss scale n_p n_l, K [9], R [9], t [3], pts_2d, pts_3d,
// line_2d, line_3d; unit weights, no masks.  Output: c [3], H [21], B [21], n_live, one number per line (%.17g).
#include <cstdio>
#include <vector>

#include "../../cvxpnpl_amd/csrc/refine_robust_auto_core.h"

int main()
{
    int loss, n_p, n_l;
    double scale, K[9], R[9], t[3];
    if (scanf("%d %lf %d %d", &loss, &scale, &n_p, &n_l) != 4 || n_p < 0 || n_l < 0) return 2;
    auto read = [](double *p, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (scanf("%lf", p + i) != 1) return false;
        return true;
    };
    std::vector<double> p2(2 * (size_t)n_p), p3(3 * (size_t)n_p), l2(4 * (size_t)n_l), l3(6 * (size_t)n_l);
    if (!read(K, 9) || !read(R, 9) || !read(t, 3) || !read(p2.data(), p2.size()) || !read(p3.data(), p3.size()) || !read(l2.data(), l2.size()) ||
        !read(l3.data(), l3.size()))
        return 2;
    cvxrb::HostLanes ln;
    ln.wp.pb.n_p = n_p; ln.wp.pb.n_l = n_l;
    ln.wp.pb.p2 = p2.data(); ln.wp.pb.p3 = p3.data(); ln.wp.pb.l2 = l2.data(); ln.wp.pb.l3 = l3.data();
    ln.wp.pb.mp = ln.wp.pb.ml = nullptr;
    ln.wp.wp = ln.wp.wl = nullptr;
    ln.wp.ow_p = ln.wp.ow_l = nullptr;
    const cvxrb::Loss l = cvxrb::make_loss(loss, scale);
    // the chart of robust_cov_problem
    cvxr::Pose ps;
    for (int i = 0; i < 9; ++i) { ps.K[i] = K[i]; ps.R[i] = R[i]; }
    double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ln.each([&](const cvxr::Rec &r, double w, int64_t) { cvxrb::wrec_centre(r, w, s6); });
    for (int i = 0; i < 3; ++i) ps.c[i] = s6[3] > 0.0 ? s6[i] / s6[3] : 0.0;
    double Rc[3];
    cvxr::rot_c(ps, Rc);
    for (int i = 0; i < 3; ++i) ps.tc[i] = Rc[i] + t[i];
    double acc[cvxrbg::ACC_N], Bm[21];
    for (double &x : acc) x = 0.0;
    for (double &x : Bm) x = 0.0;
    ln.each([&](const cvxr::Rec &r, double w, int64_t) { cvxrbg::wrec_acc_full(r, w, ps, l, acc); });
    ln.each([&](const cvxr::Rec &r, double w, int64_t) { cvxra::wrec_meat(r, w, ps, l, Bm); });
    for (int i = 0; i < 3; ++i) printf("%.17g\n", ps.c[i]);
    for (int i = 0; i < 21; ++i) printf("%.17g\n", acc[i]);
    for (int i = 0; i < 21; ++i) printf("%.17g\n", Bm[i]);
    printf("%d\n", (int)s6[4]);
    return 0;
}
