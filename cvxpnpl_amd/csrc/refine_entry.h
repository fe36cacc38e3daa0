// refine_entry.h -- what the entry points of the four refinement libraries (refine, refine_grad, refine_robust, refine_robust_grad) share
// around their kernels and cores: the error text, the argument contract of a batch call and of a scenes call, the per-problem view of the
// host forms, and the common fields of the kernels' argument blocks.  Host-only, plain C++17 (the stand-alone sanitizer programs compile
// the host_*.cpp files without HIP); what needs the HIP runtime is behind __HIPCC__.  Every function is inline and hidden: each library
// keeps a copy of its own -- its own thread-local message -- and exports nothing of this.
//
// The checks return a message or null (ransac_hip.hip's idiom); an entry point runs them in this order: the sizes, the zero-size no-op
// before any pointer is looked at, the pointers, K and the poses, its own outputs, the status column, its own options.
#pragma once
#include <stdint.h>

#include <cmath>

#include "entry_error.h"
#include "host_pool.h"
#include "refine_core.h"
#include "refine_view.h"

#define CVXRE_FN inline __attribute__((visibility("hidden")))

namespace cvxre {

// the error text: entry_error.h
using cvxee::bad_args;
using cvxee::err_buf;
#if defined(__HIPCC__)
using cvxee::launched;
#endif

// ---- the argument contract ----

// batch / scene count and the two correspondence counts; a problem of the batch form indexes its records by an int, hence `most`
CVXRE_FN const char *check_sizes(int64_t n, int64_t n_p, int64_t n_l, int64_t most = INT64_MAX)
{
    return n < 0 || n_p < 0 || n_l < 0 || n_p > most - n_l ? "negative size" : nullptr;
}

CVXRE_FN const char *check_pairs(int64_t n_p, const double *p2, const double *p3, int64_t n_l, const double *l2, const double *l3)
{
    return (n_p > 0 && (!p2 || !p3)) || (n_l > 0 && (!l2 || !l3)) ? "a correspondence pointer is null" : nullptr;
}

// the pointers of a scenes call: the offsets, then the packed correspondences
CVXRE_FN const char *check_scenes(const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines, const double *p2, const double *p3,
                                  const double *l2, const double *l3)
{
    if (!off_p || (n_lines > 0 && !off_l)) return "d_pt_offsets or d_ln_offsets is null";
    return check_pairs(n_pts, p2, p3, n_lines, l2, l3);
}

CVXRE_FN const char *check_pose(int32_t K_per, const double *K, const double *R, const double *t)
{
    if (K_per != 0 && K_per != 1) return "K_per_problem / K_per_scene is 0 or 1";
    if (!K || !R || !t) return "K, R or t is null";
    return nullptr;
}

CVXRE_FN const char *check_status(const int32_t *status, int64_t status_stride)
{
    return status && status_stride < 0 ? "negative status_stride" : nullptr;
}

// The Levenberg-Marquardt options of refine and refine_robust: the defaults into o, then -- opts given -- its size (size_what: the
// message names the library's own struct) and the three numbers both structs carry.  What else a struct holds is its library's to check.
template <class O>
CVXRE_FN const char *check_lm_opts(const O *opts, const char *size_what, cvxr::Opts &o)
{
    o.max_iters = 30; o.step_tol = 1e-10; o.lambda0 = 1e-3; o.sigma_px = 0.0;
    if (!opts) return nullptr;
    if (opts->struct_size != sizeof(O)) return size_what;
    if (opts->max_iters < 0) return "negative max_iters";
    if (!(opts->step_tol >= 0.0) || !std::isfinite(opts->step_tol)) return "step_tol is not a finite non-negative number";
    if (!(opts->lambda0 >= 0.0) || !std::isfinite(opts->lambda0)) return "lambda0 is not a finite non-negative number";
    o.max_iters = opts->max_iters; o.step_tol = opts->step_tol; o.lambda0 = opts->lambda0;
    return nullptr;
}

// loss / scale_px of refine_robust and refine_robust_grad; the kinds are CVXPNPL_LOSS_* = cvxrb::LossKind, 0 (l2) to 2
CVXRE_FN const char *check_loss(int32_t loss, double scale_px)
{
    if (loss < 0 || loss > 2) return "loss is 0 (l2), 1 (huber) or 2 (cauchy)";
    if (loss != 0 && (!(scale_px > 0.0) || !std::isfinite(scale_px))) return "scale_px is not a finite positive number";
    return nullptr;
}

// the grid of a batch launch, per_block problems to a workgroup, and of a scenes launch, one workgroup each
CVXRE_FN const char *check_batch_grid(int64_t batch, int per_block, int64_t &grid)
{
    grid = (batch + per_block - 1) / per_block;
    return grid > 0x7fffffffLL ? "batch too large for one launch" : nullptr;
}

CVXRE_FN const char *check_scenes_grid(int64_t n_scenes) { return n_scenes > 0x7fffffffLL ? "too many scenes for one launch" : nullptr; }

// ---- the host forms ----

// problem b's slice of an optional array of n records of `per` elements: null when the array is absent or the kind has no records
template <class T>
CVXRE_FN T *slice(T *p, int64_t b, int32_t n, int per = 1)
{
    return p && n > 0 ? p + b * n * per : nullptr;
}

// problem b of a host batch: its Prob with the masks (refine_view.h's batch_prob, the statement the kernels use), whether its status is
// admitted, and its K returned
CVXRE_FN const double *host_problem(int64_t b, int32_t n_p, const double *pts_2d, const double *pts_3d, int32_t n_l, const double *line_2d,
                                    const double *line_3d, const double *K, int32_t K_per_problem, const int32_t *status, int64_t status_stride,
                                    uint32_t admit_mask, const uint8_t *mask_pts, const uint8_t *mask_lines, cvxr::Prob &pb, bool &admit)
{
    admit = !status || cvxr::admitted(status[b * status_stride], admit_mask);
    return cvxr::batch_prob(b, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem, mask_pts, mask_lines, pb);
}

// ... its weights (W: cvxrb::WProb) and its gradient outputs (G: cvxrg::Grads)
template <class W>
CVXRE_FN void host_weights(W &wp, int64_t b, int32_t n_p, int32_t n_l, const double *w_pts, const double *w_lines)
{
    wp.wp = slice(w_pts, b, n_p); wp.wl = slice(w_lines, b, n_l);
}

template <class G>
CVXRE_FN void host_grads(G &g, int64_t b, int32_t n_p, int32_t n_l, double *g_pts_2d, double *g_pts_3d, double *g_line_2d, double *g_line_3d)
{
    g.p2 = slice(g_pts_2d, b, n_p, 2); g.p3 = slice(g_pts_3d, b, n_p, 3);
    g.l2 = slice(g_line_2d, b, n_l, 4); g.l3 = slice(g_line_3d, b, n_l, 6);
}

// ---- the kernels' argument blocks: the fields every BatchArgs / VjpBatchArgs and every SceneArgs / VjpSceneArgs has under these names ----

template <class A>
CVXRE_FN void fill_batch(A &a, int64_t batch, int32_t n_p, const double *p2, const double *p3, int32_t n_l, const double *l2, const double *l3,
                         const double *K, int32_t K_per_problem, const double *R, const double *t, const int32_t *status, int64_t status_stride,
                         uint32_t admit_mask, const uint8_t *mask_pts, const uint8_t *mask_lines)
{
    a.batch = batch; a.n_p = n_p; a.n_l = n_l; a.K_per_problem = K_per_problem; a.admit = admit_mask; a.status_stride = status_stride;
    a.p2 = p2; a.p3 = p3; a.l2 = l2; a.l3 = l3; a.K = K; a.R = R; a.t = t; a.status = status;
    a.mp = n_p > 0 ? mask_pts : nullptr; a.ml = n_l > 0 ? mask_lines : nullptr;
}

template <class A>
CVXRE_FN void fill_scenes(A &a, int64_t n_scenes, const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines, const double *p2,
                          const double *p3, const double *l2, const double *l3, const double *K, int32_t K_per_scene, const double *R, const double *t,
                          const int32_t *status, int64_t status_stride, uint32_t admit_mask, const uint8_t *mask_pts, const uint8_t *mask_lines)
{
    a.n_scenes = n_scenes; a.n_pts = n_pts; a.n_lines = n_lines; a.off_p = off_p; a.off_l = n_lines > 0 ? off_l : nullptr;
    a.p2 = p2; a.p3 = p3; a.l2 = l2; a.l3 = l3; a.K = K; a.R = R; a.t = t; a.K_per_scene = K_per_scene;
    a.admit = admit_mask; a.status_stride = status_stride; a.status = status;
    a.mp = n_pts > 0 ? mask_pts : nullptr; a.ml = n_lines > 0 ? mask_lines : nullptr;
}

} // namespace cvxre
