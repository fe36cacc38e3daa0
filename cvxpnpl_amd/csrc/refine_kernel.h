// refine_kernel.h -- the reprojection refinement on the device (include/cvxpnpl_amd_refine.h); the mathematics and
// the Levenberg-Marquardt loop are refine_core.h, shared with the host path.  The whole loop of a problem runs inside one launch; between
// iterations nothing goes to memory.
//   refine_group_kernel<RPL>   the batch form [B, n_p] + [B, n_l]: 16 lanes per problem, four problems per wavefront (the layout of
//       vjp_group_kernel).  Lane l owns correspondences l, l + 16, ...; with RPL = 1, 2 or 4 records per lane they are loaded ONCE into
//       registers (up to 64 correspondences), with RPL = 0 every pass reads them again (L2 serves that).  The 29 sums of a pass meet by
//       xor exchanges of width 16 and every lane solves the damped 6x6 itself.  The four groups of a wavefront run one wavefront-uniform
//       loop (refine_problem's any() is a wavefront vote); a group whose problem has ended keeps its state frozen.  No LDS.
//   refine_scenes_kernel       packed scenes (offsets, optional masks): ONE workgroup of 256 per scene, records re-read in every pass, the
//       sums through a wavefront butterfly and LDS; every lane then holds the same totals and takes the same step.  Scenes of any size;
//       a very large scene is still one workgroup.
// Both clamp what they index: a group beyond the batch works on the last problem and writes nothing, a scene's slices go through
// cvxn::scene_slice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ransac_common.h"
#include "refine_core.h"
#include "refine_lanes.h"

namespace cvxr {

struct Outputs {
    double *R, *t, *cost, *cov; // [n][9], [n][3], [n][2], [n][36] (cov optional)
    int32_t *iters, *status, *n_live;
};

// (a pose that was not refined passes through bit for bit: Rin / tin are read here, by the one lane that then writes -- they may alias the outputs)
__device__ __forceinline__ void write_result(const Outputs &o, int64_t b, const Result &res, const double *Rin, const double *tin)
{
    const bool done = res.status <= REFINE_MAXITER;
    CVX_UNROLL for (int i = 0; i < 9; ++i) o.R[9 * b + i] = done ? res.R[i] : Rin[i];
    CVX_UNROLL for (int i = 0; i < 3; ++i) o.t[3 * b + i] = done ? res.t[i] : tin[i];
    o.cost[2 * b + 1] = res.cost;
    o.iters[b] = res.iters; o.status[b] = res.status; o.n_live[b] = res.n_live;
}

struct BatchArgs {
    int64_t batch;
    int n_p, n_l, K_per_problem;
    uint32_t admit;
    int64_t status_stride;
    const double *p2, *p3, *l2, *l3, *K, *R, *t;
    const int32_t *status;
    const uint8_t *mp, *ml;
    Opts opts;
    Outputs out;
};

template <int RPL>
__global__ void __launch_bounds__(TPB) refine_group_kernel(BatchArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    const bool mine = g < a.batch;
    const int64_t b = mine ? g : a.batch - 1; // an empty group of the last wavefront shadows the last problem and writes nothing
    GroupLanes<RPL> ln;
    ln.lane = threadIdx.x & 15;
    const cvx::ProblemView pv = cvx::make_view(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem);
    ln.pb.n_p = a.n_p; ln.pb.n_l = a.n_l;
    ln.pb.p2 = pv.p2; ln.pb.p3 = pv.p3; ln.pb.l2 = pv.l2; ln.pb.l3 = pv.l3;
    ln.pb.mp = a.mp ? a.mp + b * a.n_p : nullptr;
    ln.pb.ml = a.ml ? a.ml + b * a.n_l : nullptr;
    ln.load();
    const bool admit = mine && (!a.status || admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.lane == 0;
    Result res;
    refine_problem(ln, pv.K, a.R + 9 * b, a.t + 3 * b, admit, a.opts, res, writer ? a.out.cost + 2 * b : nullptr);
    if (writer) write_result(a.out, b, res, a.R + 9 * b, a.t + 3 * b);
}

// the covariance of the batch form, after refine_group_kernel on the same stream: reads the refined poses and their statuses
__global__ void __launch_bounds__(TPB) cov_group_kernel(BatchArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return; // whole groups: the exchanges stay inside a group
    GroupLanes<0> ln;
    ln.lane = threadIdx.x & 15;
    const cvx::ProblemView pv = cvx::make_view(g, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem);
    ln.pb.n_p = a.n_p; ln.pb.n_l = a.n_l;
    ln.pb.p2 = pv.p2; ln.pb.p3 = pv.p3; ln.pb.l2 = pv.l2; ln.pb.l3 = pv.l3;
    ln.pb.mp = a.mp ? a.mp + g * a.n_p : nullptr;
    ln.pb.ml = a.ml ? a.ml + g * a.n_l : nullptr;
    covariance_problem(ln, pv.K, a.out.R + 9 * g, a.out.t + 3 * g, a.out.status[g], a.out.cost[2 * g + 1], a.out.n_live[g], a.opts,
                       ln.lane == 0 ? a.out.cov + 36 * g : nullptr);
}

struct SceneArgs {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l; // [n_scenes + 1]; off_l may be null (no lines)
    const double *p2, *p3, *l2, *l3, *K, *R, *t;
    int K_per_scene;
    uint32_t admit;
    int64_t status_stride;
    const int32_t *status;
    const uint8_t *mp, *ml;       // [n_pts], [n_lines], optional
    Opts opts;
    Outputs out;
};

// the workgroup's scene: both slices clamped, K / R / t staged in LDS (read from LDS they are per-lane values; read through a uniform pointer,
// the pose and everything computed from it would crowd the scalar registers).  R, t: the poses to stage, [n_scenes][9] / [n_scenes][3].
__device__ __forceinline__ void scene_lanes(const SceneArgs &a, int64_t f, const double *R, const double *t, double *red, double *pose, BlockLanes &ln)
{
    if (threadIdx.x < 9) pose[threadIdx.x] = a.K[(a.K_per_scene ? f * 9 : 0) + threadIdx.x];
    else if (threadIdx.x < 18) pose[threadIdx.x] = R[9 * f + threadIdx.x - 9];
    else if (threadIdx.x < 21) pose[threadIdx.x] = t[3 * f + threadIdx.x - 18];
    __syncthreads();
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts);
    cvxn::Slice sl{0, 0};
    if (a.off_l) sl = cvxn::scene_slice(a.off_l, f, a.n_lines);
    ln.red = red;
    ln.pb.n_p = sp.n;
    ln.pb.n_l = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    ln.pb.p2 = a.p2 + sp.beg * 2; ln.pb.p3 = a.p3 + sp.beg * 3; // (never followed where the slice is empty)
    ln.pb.l2 = a.l2 + sl.beg * 4; ln.pb.l3 = a.l3 + sl.beg * 6;
    ln.pb.mp = a.mp ? a.mp + sp.beg : nullptr;
    ln.pb.ml = a.ml ? a.ml + sl.beg : nullptr;
}

__global__ void __launch_bounds__(TPB) refine_scenes_kernel(SceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[21];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    BlockLanes ln;
    scene_lanes(a, f, a.R, a.t, red, pose, ln);
    const bool admit = !a.status || admitted(a.status[f * a.status_stride], a.admit);
    Result res;
    const double *ps = pose;
    refine_problem(ln, ps, ps + 9, ps + 18, admit, a.opts, res, threadIdx.x == 0 ? a.out.cost + 2 * f : nullptr);
    if (threadIdx.x == 0) write_result(a.out, f, res, ps + 9, ps + 18);
}

// the covariance of the scenes, after refine_scenes_kernel on the same stream: reads the refined poses and their statuses
__global__ void __launch_bounds__(TPB) cov_scenes_kernel(SceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[21];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    BlockLanes ln;
    scene_lanes(a, f, a.out.R, a.out.t, red, pose, ln);
    const double *ps = pose;
    covariance_problem(ln, ps, ps + 9, ps + 18, a.out.status[f], a.out.cost[2 * f + 1], a.out.n_live[f], a.opts,
                       threadIdx.x == 0 ? a.out.cov + 36 * f : nullptr);
}

} // namespace cvxr
