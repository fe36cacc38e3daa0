// ransac_pnpl_lo_core.h -- the rules of local optimisation in adaptive RANSAC over points AND lines
// (include/cvxpnpl_amd_ransac_pnpl_lo.h), ONE statement of them for the device (lo_assemble_pnpl_active_kernel,
// lo_update_pnpl_active_kernel) and the host (cvxpnpl_ransac_pnpl_lo_assemble_host).  What section 24 states for points -- the camera, the
// point predicate and take_fit -- is ransac_lo_core.h as it stands, the centre, the order of the sums and the finish are
// ransac_assemble_core.h; here is what lines add.
//
// The assembly of one active entry, by LANES = 256 lanes in four wavefronts:
//   taken point m = cvxn::is_inlier at the scene's running pose, threshold (thresh * m_k)^2                      (cvxnlo::taken)
//   taken line m  = cvxnl::is_line_inlier, threshold thresh * m_k: the image line normalised ONCE, then both end points in front of the
//                   camera and within the threshold of it                                                         (line_taken)
//   centre        = cvxas::centre of the first three taken 3D RECORDS in the order "points, then lines", a line giving its two end
//                   points: up to three points, then -- while fewer than three records -- cvxas::centre_lines_wanted lines
//   lane l        adds its taken points l, l + 256, ... and then its taken lines l, l + 256, ... into the same 60 sums  (lane_sums)
//   a wave, the entry: the XOR butterfly and the wave order of ransac_assemble_core.h
// so the 60 sums depend on the inputs alone.  On the device the scene and the line predicate ARE cvxnl::scene_of and cvxnl::is_line_inlier;
// those are device-only, so the host build restates them expression by expression (as ransac_lo_core.h does for the point predicate).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_adaptive_core.h"
#include "ransac_common.h"
#include "ransac_lo_core.h"
#include "ransac_pnpl_common.h"
#include "solver_core.h"

namespace cvxnllo {

using cvxnlo::GRAM;
using cvxnlo::LANES;
using cvxnlo::WAVES;

// ---- scene f of a scene set: both slices clamped, L cut so that P + L fits an int32
__host__ __device__ inline cvxnl::Scene scene(const cvxnl::SceneSet &s, int64_t f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return cvxnl::scene_of(s, f);
#else
    const cvxn::Slice sp = cvxn::scene_slice(s.off_p, f, s.n_pts), sl = cvxn::scene_slice(s.off_l, f, s.n_lines);
    cvxnl::Scene sc;
    sc.P = sp.n;
    sc.L = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    sc.beg_p = sp.beg; sc.beg_l = sl.beg;
    sc.p2 = s.p2 + sp.beg * 2; sc.p3 = s.p3 + sp.beg * 3;
    sc.l2 = s.l2 + sl.beg * 4; sc.l3 = s.l3 + sl.beg * 6;
    sc.K = s.K + (s.K_per_scene ? f * 9 : 0);
    return sc;
#endif
}

// ---- the line predicate: line m of the scene's packed l2 (u0 v0 u1 v1) / l3 (P0 P1) under the camera c, threshold th (pixels)
#if !defined(__HIP_DEVICE_COMPILE__)
inline bool host_end_point_near(const cvxn::Camera &c, const double *l, double X, double Y, double Z, double thresh)
{
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double d = l[0] * (u / w) + l[1] * (v / w) + l[2];
    return depth > 0.0 && (fabs(d) < thresh);
}
#endif
__host__ __device__ inline bool line_taken(const cvxn::Camera &c, const double *l2, const double *l3, int64_t m, double th)
{
    const double *x = l2 + 4 * m, *e = l3 + 6 * m;
    const double ab[4] = {x[0], x[1], x[2], x[3]}, es[6] = {e[0], e[1], e[2], e[3], e[4], e[5]};
#if defined(__HIP_DEVICE_COMPILE__)
    return cvxnl::is_line_inlier(c, ab, es, th); // (image_line once per line, then end_point_near twice)
#else
    const double l0 = ab[1] - ab[3], l1 = ab[2] - ab[0], lc = ab[0] * ab[3] - ab[1] * ab[2];
    const double inv = 1.0 / hypot(l0, l1);
    const double l[3] = {l0 * inv, l1 * inv, lc * inv};
    return host_end_point_near(c, l, es[0], es[1], es[2], th) && host_end_point_near(c, l, es[3], es[4], es[5], th);
#endif
}

// ---- T = n n^T (packed 00 01 02 11 12 22) of a 2D line, n the normalised cross product of its two back-projected samples: the first half
// of cvx::gram_add_line, expression by expression, so that lane_sums can add the line's two end points in a ROLLED loop (one copy of the
// 60 accumulations for lines, not two)
__host__ __device__ inline void line_T(const double *Ki, const double *ab /* u0 v0 u1 v1 */, double *T)
{
    double a[3], b[3];
    cvx::bearing(Ki, ab[0], ab[1], a);
    cvx::bearing(Ki, ab[2], ab[3], b);
    double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double inv = cvx::rsqrt_(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    n[0] *= inv; n[1] *= inv; n[2] *= inv;
    T[0] = n[0] * n[0]; T[1] = n[0] * n[1]; T[2] = n[0] * n[2]; T[3] = n[1] * n[1]; T[4] = n[1] * n[2]; T[5] = n[2] * n[2];
}

// ---- lane l of an assembly: the Gram sums of the taken points l, l + LANES, ... and then of the taken lines l, l + LANES, ... about the
// centre c; returns their number (a line counts once).  th2 = th * th, handed in so that every lane squares it once.
__host__ __device__ inline int lane_sums(int l, const cvxnl::Scene &sc, const cvxn::Camera &cam, double th, double th2, const double *Ki,
                                         const double *c, cvx::Gram &g)
{
    cvx::gram_zero(g);
    int cnt = 0;
    for (int64_t m = l; m < sc.P; m += LANES) {
        if (!cvxnlo::taken(cam, sc.p2, sc.p3, m, th2)) continue;
        cvx::gram_add_point(g, Ki, sc.p2[2 * m], sc.p2[2 * m + 1], sc.p3[3 * m] - c[0], sc.p3[3 * m + 1] - c[1], sc.p3[3 * m + 2] - c[2]);
        ++cnt;
    }
#pragma unroll 1
    for (int64_t m = l; m < sc.L; m += LANES) {
        if (!line_taken(cam, sc.l2, sc.l3, m, th)) continue;
        const double *x = sc.l2 + 4 * m, *e = sc.l3 + 6 * m;
        const double ab[4] = {x[0], x[1], x[2], x[3]};
        double T[6];
        line_T(Ki, ab, T);
#pragma unroll 1
        for (int k = 0; k < 2; ++k) // cvx::gram_add_line: P0, then P1 (rolled: the body repeats)
            cvx::gram_add(g, T, e[3 * k] - c[0], e[3 * k + 1] - c[1], e[3 * k + 2] - c[2]);
        ++cnt;
    }
    return cnt;
}

} // namespace cvxnllo
