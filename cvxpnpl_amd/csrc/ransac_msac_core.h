// ransac_msac_core.h -- the arithmetic of MSAC scoring (include/cvxpnpl_amd_ransac_msac.h), ONE statement of it for
// the device (score_scenes_msac_kernel, score_active_msac_kernel, the two arg-max kernels) and the host
// (cvxpnpl_ransac_msac_score_host): the camera of a pose, the term of one correspondence, the gain of a sum, the usable rule and the
// ordering of two hypotheses.  The camera and the predicate restate cvxn::camera_load and cvxn::is_inlier (ransac_common.h) expression
// by expression -- those are device-only and pinned by the resource tables of five libraries, so they are not touched -- and a count
// made here is the count made there.
//
//   gain(h) = ( sum over the scene's points that pass the predicate of (th2 - r2) ) / th2,   th2 = thresh^2,  r2 = du^2 + dv^2
//
// Every term is positive, so nothing cancels; the sum runs serially in scene order, so the gain of a pose over a scene is a function of
// the inputs alone.  gain lies in [0, count]; maximising it minimises sum min(r2, th2), a point behind the camera costing th2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvxnm {

struct Cam {
    double M[12];      // K R | K t : pixel-space projection
    double r2[3], t2;  // depth row
};
__host__ __device__ inline void cam_load(const double *Rp, const double *tp, const double *Kp, Cam &c)
{
    double R[9], t[3], K[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = Rp[i]; K[i] = Kp[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.M[i * 4 + j] = K[i * 3] * R[j] + K[i * 3 + 1] * R[3 + j] + K[i * 3 + 2] * R[6 + j];
        c.M[i * 4 + 3] = K[i * 3] * t[0] + K[i * 3 + 1] * t[1] + K[i * 3 + 2] * t[2];
    }
    c.r2[0] = R[6]; c.r2[1] = R[7]; c.r2[2] = R[8]; c.t2 = t[2];
}

// one correspondence under one pose: whether it passes the inlier predicate (depth > 0 and r2 < th2; a NaN compares false) and th2 - r2
struct Term { bool in; double g; };
__host__ __device__ inline Term point_gain(const Cam &c, double X, double Y, double Z, double x, double y, double th2)
{
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double du = u / w - x, dv = v / w - y;
    const double r2 = du * du + dv * dv;
    return Term{depth > 0.0 && (r2 < th2), th2 - r2};
}

// the running sum of a pose: terms are added in the order they are given
struct Sum { double s; int32_t n; };
__host__ __device__ inline void sum_add(Sum &a, bool usable, Term p)
{
    const bool in = usable && p.in;
    a.s += in ? p.g : 0.0;
    a.n += in ? 1 : 0;
}
// ... and its gain: the one division.  No inlier (and so thresh = 0): exactly 0.
__host__ __device__ inline double sum_gain(const Sum &a, double th2) { return a.n > 0 ? a.s / th2 : 0.0; }

// the usable rule of cvxn::hypothesis_usable: a lane past the end scores nothing, nor does a status outside usable_mask
__host__ __device__ inline bool hypothesis_usable(bool live, const int32_t *status, int64_t g, uint32_t usable_mask)
{
    bool usable = live;
    if (live && status) {
        const int32_t s = status[g];
        usable = s >= 0 && s < 32 && ((usable_mask >> s) & 1u);
    }
    return usable;
}

// ---- the ordering: a gain that is not > 0 (negative, NaN) is read as 0; the higher gain is better, then the lower index
__host__ __device__ inline double gain_read(double g) { return g > 0.0 ? g : 0.0; }
__host__ __device__ inline bool better(double gain_a, int32_t h_a, double gain_b, int32_t h_b)
{
    const double a = gain_read(gain_a), b = gain_read(gain_b);
    return a > b || (a == b && h_a < h_b);
}

} // namespace cvxnm
