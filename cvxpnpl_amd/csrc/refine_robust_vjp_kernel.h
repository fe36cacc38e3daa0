// refine_robust_vjp_kernel.h -- the VJP of the robust reprojection minimum on the device (include/cvxpnpl_amd_refine_robust_grad.h,
// DESIGN.md section 18); the mathematics is refine_robust_vjp_core.h, shared with the host path, over the weighted lane classes of
// refine_robust_kernel.h (WGroupLanes<RPL>, WBlockLanes: a record, its weight and its index).  Two passes over a problem's records inside
// one launch, as in refine_vjp_kernel.h: the reduction of the full Hessian, and -- after every lane has solved the 6x6 -- the gradients
// of the records the lane owns and of their weights.  No loop over iterations, no vote.
//   refine_robust_vjp_group_kernel<RPL>   the batch form: 16 lanes per problem, four problems per wavefront.  RPL = 1, 2 or 4 records
//       per lane stay in registers with their weights between the two passes, RPL = 0 reads them again.  xor exchanges of width 16, no
//       LDS.  An empty group of the last wavefront shadows the last problem and writes nothing.
//   refine_robust_vjp_scenes_kernel       packed scenes: one workgroup of 256 per scene; K, R, t, the upstream gradient and scale_px
//       staged in LDS.
// Both clamp what they index; the views, the scenes' gradient slices and the staging are refine_view.h's, the weights' slices
// refine_robust_kernel.h's weighted_prob.  (refine_robust_kernel.h's three kernels that are not templates ride along into this library's
// code object; nothing here launches them.)
#pragma once
#include "refine_lanes.h"
#include "refine_robust_kernel.h"
#include "refine_robust_vjp_core.h"
#include "refine_view.h"

namespace cvxrbg {

using cvxr::POSE_N;
using cvxr::TPB;
using cvxr::UPSTREAM_N;
using cvxr::WAVES;
using cvxrb::in_vgpr;

struct VjpBatchArgs {
    int64_t batch;
    int n_p, n_l, K_per_problem;
    uint32_t admit;
    int64_t status_stride;
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *wp, *wl, *gR, *gt;
    const int32_t *status;
    const uint8_t *mp, *ml;
    Loss loss;       // made on the host: uniform, it stays in scalar registers, of which these kernels have enough (the vector ones are full)
    double *g_p2, *g_p3, *g_l2, *g_l3, *g_wp, *g_wl, *info;
    int32_t *vstatus;
};

template <int RPL>
__global__ void __launch_bounds__(TPB) refine_robust_vjp_group_kernel(VjpBatchArgs a)
{
    const int64_t gi = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    const bool mine = gi < a.batch;
    const int64_t b = mine ? gi : a.batch - 1; // an empty group of the last wavefront shadows the last problem and writes nothing
    cvxrb::WGroupLanes<RPL> ln;
    ln.g.lane = threadIdx.x & 15;
    WProb &wp = ln.wp;
    const double *K = cvxrb::weighted_prob(a, b, wp);
    wp.ow_p = a.g_wp ? a.g_wp + b * a.n_p : nullptr; // (the weights' gradients: refine_robust_vjp_core.h)
    wp.ow_l = a.g_wl ? a.g_wl + b * a.n_l : nullptr;
    ln.load();
    const bool admit = mine && (!a.status || cvxr::admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.g.lane == 0;
    Grads g;
    g.p2 = a.g_p2 ? a.g_p2 + b * a.n_p * 2 : nullptr;
    g.p3 = a.g_p3 ? a.g_p3 + b * a.n_p * 3 : nullptr;
    g.l2 = a.g_l2 ? a.g_l2 + b * a.n_l * 4 : nullptr;
    g.l3 = a.g_l3 ? a.g_l3 + b * a.n_l * 6 : nullptr;
    const int st = robust_vjp_problem(ln, wp, K, a.R + 9 * b, a.t + 3 * b, a.gR ? a.gR + 9 * b : nullptr, a.gt ? a.gt + 3 * b : nullptr, admit, mine, a.loss, g, writer && a.info ? a.info + 2 * b : nullptr);
    if (writer) a.vstatus[b] = st;
}

struct VjpSceneArgs {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l; // [n_scenes + 1]; off_l may be null (no lines)
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *wp, *wl, *gR, *gt;
    int K_per_scene;
    uint32_t admit;
    int64_t status_stride;
    const int32_t *status;
    const uint8_t *mp, *ml;       // [n_pts], [n_lines], optional
    int loss_kind;
    double scale_px;
    double *g_p2, *g_p3, *g_l2, *g_l3, *g_wp, *g_wl, *info;
    int32_t *vstatus;
};

__global__ void __launch_bounds__(TPB) refine_robust_vjp_scenes_kernel(VjpSceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    constexpr int SCALE_AT = POSE_N + UPSTREAM_N;
    __shared__ double pose[SCALE_AT + 1]; // K, R, t, the upstream gradients G_R, g_t (refine_view.h), scale_px
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    const double *gR = a.gR, *gt = a.gt, scale_px = a.scale_px; // (captured as values: refine_vjp_kernel.h)
    cvxr::stage_pose(a.K, a.K_per_scene, a.R, a.t, f, pose, [&] {
        cvxr::stage_upstream(gR, gt, f, pose, [&] { if (threadIdx.x == SCALE_AT) pose[SCALE_AT] = scale_px; });
    });
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts), sl = cvxr::line_slice(a.off_l, f, a.n_lines);
    cvxrb::WBlockLanes ln;
    ln.b.red = red;
    WProb &wp = ln.wp;
    cvxr::scene_prob(sp, sl, a.p2, a.p3, a.l2, a.l3, a.mp, a.ml, wp.pb);
    // (this kernel's scalar registers are full where its vector ones are not: the six pointers that the weights add live in vector
    // registers -- refine_robust_kernel.h's in_vgpr)
    wp.wp = in_vgpr(a.wp ? a.wp + sp.beg : nullptr);
    wp.wl = in_vgpr(a.wl ? a.wl + sl.beg : nullptr);
    wp.ow_p = in_vgpr(a.g_wp ? a.g_wp + sp.beg : nullptr);
    wp.ow_l = in_vgpr(a.g_wl ? a.g_wl + sl.beg : nullptr);
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    Grads g;
    cvxr::scene_grads(sp, sl, a.g_p2, a.g_p3, a.g_l2, a.g_l3, g);
    const double *ps = pose;
    const int st = robust_vjp_problem(ln, wp, ps, ps + 9, ps + 18, ps + POSE_N, ps + POSE_N + 9, admit, true, cvxrb::make_loss(a.loss_kind, ps[SCALE_AT]), g,
                                      threadIdx.x == 0 && a.info ? a.info + 2 * f : nullptr);
    if (threadIdx.x == 0) a.vstatus[f] = st;
}

} // namespace cvxrbg
