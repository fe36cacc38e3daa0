// refine_vjp_kernel.h -- the VJP of the reprojection minimum on the device (include/cvxpnpl_amd_refine_grad.h); the
// mathematics is refine_vjp_core.h, shared with the host path, over the lane classes of refine_lanes.h.  Two passes over a problem's
// records inside one launch: the reduction of the full Hessian, and -- after every lane has solved the 6x6 -- the gradients of the records
// the lane owns.  No loop over iterations, no vote.
//   refine_vjp_group_kernel<RPL>   the batch form: 16 lanes per problem, four problems per wavefront.  Lane l owns records l, l + 16, ...;
//       RPL = 1, 2 or 4 records per lane stay in registers between the two passes, RPL = 0 reads them again.  The 28 sums meet by xor
//       exchanges of width 16.  An empty group of the last wavefront shadows the last problem and writes nothing.  No LDS.
//   refine_vjp_scenes_kernel       packed scenes: one workgroup of 256 per scene, K / R / t and the upstream gradient staged in LDS, the
//       sums through BlockLanes' butterfly -> LDS -> fixed-order add; each thread then writes the gradients of the records it owns.
// Both clamp what they index, as the kernels of refine_kernel.h do; the views, the scenes' gradient slices and the staging are
// refine_view.h's (a batch problem's gradient slices stay here: as a function they changed the registers of all four group kernels).
#pragma once
#include "refine_lanes.h"
#include "refine_view.h"
#include "refine_vjp_core.h"

namespace cvxrg {

using cvxr::POSE_N;
using cvxr::TPB;
using cvxr::UPSTREAM_N;
using cvxr::WAVES;

struct VjpBatchArgs {
    int64_t batch;
    int n_p, n_l, K_per_problem;
    uint32_t admit;
    int64_t status_stride;
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *gR, *gt;
    const int32_t *status;
    const uint8_t *mp, *ml;
    double *g_p2, *g_p3, *g_l2, *g_l3, *info;
    int32_t *vstatus;
};

template <int RPL>
__global__ void __launch_bounds__(TPB) refine_vjp_group_kernel(VjpBatchArgs a)
{
    const int64_t gi = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    const bool mine = gi < a.batch;
    const int64_t b = mine ? gi : a.batch - 1; // an empty group of the last wavefront shadows the last problem and writes nothing
    cvxr::GroupLanes<RPL> ln;
    ln.lane = threadIdx.x & 15;
    const double *K = cvxr::batch_prob(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem, a.mp, a.ml, ln.pb);
    ln.load();
    const bool admit = mine && (!a.status || cvxr::admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.lane == 0;
    Grads g;
    g.p2 = a.g_p2 ? a.g_p2 + b * a.n_p * 2 : nullptr;
    g.p3 = a.g_p3 ? a.g_p3 + b * a.n_p * 3 : nullptr;
    g.l2 = a.g_l2 ? a.g_l2 + b * a.n_l * 4 : nullptr;
    g.l3 = a.g_l3 ? a.g_l3 + b * a.n_l * 6 : nullptr;
    const int st = vjp_problem(ln, ln.lane, 16, K, a.R + 9 * b, a.t + 3 * b, a.gR ? a.gR + 9 * b : nullptr, a.gt ? a.gt + 3 * b : nullptr, admit, mine,
                               g, writer && a.info ? a.info + 2 * b : nullptr);
    if (writer) a.vstatus[b] = st;
}

struct VjpSceneArgs {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l; // [n_scenes + 1]; off_l may be null (no lines)
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *gR, *gt;
    int K_per_scene;
    uint32_t admit;
    int64_t status_stride;
    const int32_t *status;
    const uint8_t *mp, *ml;       // [n_pts], [n_lines], optional
    double *g_p2, *g_p3, *g_l2, *g_l3, *info;
    int32_t *vstatus;
};

__global__ void __launch_bounds__(TPB) refine_vjp_scenes_kernel(VjpSceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[POSE_N + UPSTREAM_N]; // K, R, t, then the upstream gradients G_R, g_t (refine_view.h)
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    const double *gR = a.gR, *gt = a.gt; // (captured as values: nothing here takes the address of the argument block -- refine_view.h)
    cvxr::stage_pose(a.K, a.K_per_scene, a.R, a.t, f, pose, [&] { cvxr::stage_upstream(gR, gt, f, pose, [] {}); });
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts), sl = cvxr::line_slice(a.off_l, f, a.n_lines);
    cvxr::BlockLanes ln;
    ln.red = red;
    cvxr::scene_prob(sp, sl, a.p2, a.p3, a.l2, a.l3, a.mp, a.ml, ln.pb);
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    Grads g;
    cvxr::scene_grads(sp, sl, a.g_p2, a.g_p3, a.g_l2, a.g_l3, g);
    const double *ps = pose;
    const int st = vjp_problem(ln, (int)threadIdx.x, TPB, ps, ps + 9, ps + 18, ps + POSE_N, ps + POSE_N + 9, admit, true, g,
                               threadIdx.x == 0 && a.info ? a.info + 2 * f : nullptr);
    if (threadIdx.x == 0) a.vstatus[f] = st;
}

} // namespace cvxrg
