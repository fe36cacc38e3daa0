// devsim.hip -- TEST-ONLY device twin of tests/hostsim/hostsim.cpp: the probe kernels of devsim_body.h over the headers as the solver
// library's unit (csrc/cvxpnpl_hip.hip) compiles them, plus the pieces only that unit has: cvxw::fast_rcp (wave_kernel.h) and the quad
// kernel's rotation parameters cvxq::pair_cs / pair_cs_f64 (quad_kernel.h).  Never imported by the cvxpnpl_amd package; built by
// tests/devsim/__init__.py.
#define DS(name) ds_##name
#include "devsim_body.h"

#include "wave_kernel.h"
#include "quad_kernel.h"

namespace {

__global__ void k_fast_rcp(const double *x, double *y, int n)
{
    DS_LANE(n);
    y[i] = cvxw::fast_rcp(x[i]);
}
// (d, gam, rot, tie_neg) -> (c, s, t)
__global__ void k_pair_f32(const float *dg, const int *rot, const int *tie, float *out, int n)
{
    DS_LANE(n);
    float c, s, t;
    cvxq::pair_cs(dg[2 * i], dg[2 * i + 1], rot[i] != 0, tie[i] != 0, c, s, t);
    out[3 * i] = c; out[3 * i + 1] = s; out[3 * i + 2] = t;
}
// (d, gam, rot, tie_neg) -> (c, s, dl)
__global__ void k_pair_f64(const double *dg, const int *rot, const int *tie, double *out, int n)
{
    DS_LANE(n);
    double c, s, dl;
    cvxq::pair_cs_f64(dg[2 * i], dg[2 * i + 1], rot[i] != 0, tie[i] != 0, c, s, dl);
    out[3 * i] = c; out[3 * i + 1] = s; out[3 * i + 2] = dl;
}

} // namespace

extern "C" {
int ds_fast_rcp(const double *x, double *y, int n) { DS_LAUNCH(k_fast_rcp, n, x, y, n); }
int ds_pair_f32(const float *dg, const int *rot, const int *tie, float *out, int n) { DS_LAUNCH(k_pair_f32, n, dg, rot, tie, out, n); }
int ds_pair_f64(const double *dg, const int *rot, const int *tie, double *out, int n) { DS_LAUNCH(k_pair_f64, n, dg, rot, tie, out, n); }
}
