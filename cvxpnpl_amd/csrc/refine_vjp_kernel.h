// refine_vjp_kernel.h -- the VJP of the reprojection minimum on the device (include/cvxpnpl_amd_refine_grad.h); the
// mathematics is refine_vjp_core.h, shared with the host path, over the lane classes of refine_lanes.h.  Two passes over a problem's
// records inside one launch: the reduction of the full Hessian, and -- after every lane has solved the 6x6 -- the gradients of the records
// the lane owns.  No loop over iterations, no vote.
//   refine_vjp_group_kernel<RPL>   the batch form: 16 lanes per problem, four problems per wavefront.  Lane l owns records l, l + 16, ...;
//       RPL = 1, 2 or 4 records per lane stay in registers between the two passes, RPL = 0 reads them again.  The 28 sums meet by xor
//       exchanges of width 16.  An empty group of the last wavefront shadows the last problem and writes nothing.  No LDS.
//   refine_vjp_scenes_kernel       packed scenes: one workgroup of 256 per scene, K / R / t and the upstream gradient staged in LDS, the
//       sums through BlockLanes' butterfly -> LDS -> fixed-order add; each thread then writes the gradients of the records it owns.
// Both clamp what they index, as the kernels of refine_kernel.h do.
#pragma once
#include "ransac_common.h"
#include "refine_lanes.h"
#include "refine_vjp_core.h"

namespace cvxrg {

using cvxr::TPB;
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
    const cvx::ProblemView pv = cvx::make_view(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem);
    ln.pb.n_p = a.n_p; ln.pb.n_l = a.n_l;
    ln.pb.p2 = pv.p2; ln.pb.p3 = pv.p3; ln.pb.l2 = pv.l2; ln.pb.l3 = pv.l3;
    ln.pb.mp = a.mp ? a.mp + b * a.n_p : nullptr;
    ln.pb.ml = a.ml ? a.ml + b * a.n_l : nullptr;
    ln.load();
    const bool admit = mine && (!a.status || cvxr::admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.lane == 0;
    Grads g;
    g.p2 = a.g_p2 ? a.g_p2 + b * a.n_p * 2 : nullptr;
    g.p3 = a.g_p3 ? a.g_p3 + b * a.n_p * 3 : nullptr;
    g.l2 = a.g_l2 ? a.g_l2 + b * a.n_l * 4 : nullptr;
    g.l3 = a.g_l3 ? a.g_l3 + b * a.n_l * 6 : nullptr;
    const int st = vjp_problem(ln, ln.lane, 16, pv.K, a.R + 9 * b, a.t + 3 * b, a.gR ? a.gR + 9 * b : nullptr, a.gt ? a.gt + 3 * b : nullptr, admit, mine,
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
    __shared__ double pose[33]; // K, R, t, then the upstream gradients G_R, g_t: read from LDS they are per-lane values (refine_kernel.h)
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    if (threadIdx.x < 9) pose[threadIdx.x] = a.K[(a.K_per_scene ? f * 9 : 0) + threadIdx.x];
    else if (threadIdx.x < 18) pose[threadIdx.x] = a.R[9 * f + threadIdx.x - 9];
    else if (threadIdx.x < 21) pose[threadIdx.x] = a.t[3 * f + threadIdx.x - 18];
    else if (threadIdx.x < 30) pose[threadIdx.x] = a.gR ? a.gR[9 * f + threadIdx.x - 21] : 0.0;
    else if (threadIdx.x < 33) pose[threadIdx.x] = a.gt ? a.gt[3 * f + threadIdx.x - 30] : 0.0;
    __syncthreads();
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts);
    cvxn::Slice sl{0, 0};
    if (a.off_l) sl = cvxn::scene_slice(a.off_l, f, a.n_lines);
    cvxr::BlockLanes ln;
    ln.red = red;
    ln.pb.n_p = sp.n;
    ln.pb.n_l = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    ln.pb.p2 = a.p2 + sp.beg * 2; ln.pb.p3 = a.p3 + sp.beg * 3; // (never followed where the slice is empty)
    ln.pb.l2 = a.l2 + sl.beg * 4; ln.pb.l3 = a.l3 + sl.beg * 6;
    ln.pb.mp = a.mp ? a.mp + sp.beg : nullptr;
    ln.pb.ml = a.ml ? a.ml + sl.beg : nullptr;
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    Grads g;
    g.p2 = a.g_p2 ? a.g_p2 + sp.beg * 2 : nullptr;
    g.p3 = a.g_p3 ? a.g_p3 + sp.beg * 3 : nullptr;
    g.l2 = a.g_l2 ? a.g_l2 + sl.beg * 4 : nullptr;
    g.l3 = a.g_l3 ? a.g_l3 + sl.beg * 6 : nullptr;
    const double *ps = pose;
    const int st = vjp_problem(ln, (int)threadIdx.x, TPB, ps, ps + 9, ps + 18, ps + 21, ps + 30, admit, true, g,
                               threadIdx.x == 0 && a.info ? a.info + 2 * f : nullptr);
    if (threadIdx.x == 0) a.vstatus[f] = st;
}

} // namespace cvxrg
