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
// Both clamp what they index: a group beyond the batch works on the last problem and writes nothing, a scene's slices are clamped.  The
// view of a problem or a scene, and the staging of its pose, are refine_view.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine_core.h"
#include "refine_lanes.h"
#include "refine_view.h"

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
    const double *K = batch_prob(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem, a.mp, a.ml, ln.pb);
    ln.load();
    const bool admit = mine && (!a.status || admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.lane == 0;
    Result res;
    refine_problem(ln, K, a.R + 9 * b, a.t + 3 * b, admit, a.opts, res, writer ? a.out.cost + 2 * b : nullptr);
    if (writer) write_result(a.out, b, res, a.R + 9 * b, a.t + 3 * b);
}

// the covariance of the batch form, after refine_group_kernel on the same stream: reads the refined poses and their statuses
__global__ void __launch_bounds__(TPB) cov_group_kernel(BatchArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return; // whole groups: the exchanges stay inside a group
    GroupLanes<0> ln;
    ln.lane = threadIdx.x & 15;
    const double *K = batch_prob(g, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem, a.mp, a.ml, ln.pb);
    covariance_problem(ln, K, a.out.R + 9 * g, a.out.t + 3 * g, a.out.status[g], a.out.cost[2 * g + 1], a.out.n_live[g], a.opts,
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

// the workgroup's scene: the poses R, t ([n_scenes][9] / [n_scenes][3]) staged in LDS with K, the scene's records into the lanes
__device__ __forceinline__ void scene_lanes(const SceneArgs &a, int64_t f, const double *R, const double *t, double *red, double *pose, BlockLanes &ln)
{
    stage_pose(a.K, a.K_per_scene, R, t, f, pose, [] {});
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts), sl = line_slice(a.off_l, f, a.n_lines);
    ln.red = red;
    scene_prob(sp, sl, a.p2, a.p3, a.l2, a.l3, a.mp, a.ml, ln.pb);
}

__global__ void __launch_bounds__(TPB) refine_scenes_kernel(SceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[POSE_N];
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
    __shared__ double pose[POSE_N];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    BlockLanes ln;
    scene_lanes(a, f, a.out.R, a.out.t, red, pose, ln);
    const double *ps = pose;
    covariance_problem(ln, ps, ps + 9, ps + 18, a.out.status[f], a.out.cost[2 * f + 1], a.out.n_live[f], a.opts,
                       threadIdx.x == 0 ? a.out.cov + 36 * f : nullptr);
}

} // namespace cvxr
