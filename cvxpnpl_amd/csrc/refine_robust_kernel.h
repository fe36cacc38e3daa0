// refine_robust_kernel.h -- the robust reprojection refinement on the device (include/cvxpnpl_amd_refine_robust.h);
// the mathematics and the loop are refine_robust_core.h, shared with the host path; the lanes' exchanges are refine_lanes.h's.
//   refine_robust_group_kernel<RPL>   the batch form: 16 lanes per problem, four problems per wavefront, no LDS, the wavefront vote of
//       refine_group_kernel.  A lane's register copy of a record is refine_lanes.h's Rec plus its weight.
//   refine_robust_scenes_kernel       packed scenes: one workgroup of 256 per scene.
//   robust_w_group_kernel / robust_w_scenes_kernel   rho'(s_k) per record and the inlier count at the returned pose: a pass of its own on the
//       same stream after the loop kernel (as the covariance of refine_kernel.h is), re-reading the records.
// All clamp what they index: a group beyond the batch works on the last problem and writes nothing, a scene's slices are clamped.  The
// view of a problem or a scene, and the staging of its pose, are refine_view.h's; this header adds the weights and the per-record output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine_lanes.h"
#include "refine_robust_core.h"
#include "refine_view.h"

namespace cvxrb {

using cvxr::POSE_N;
using cvxr::TPB;
using cvxr::WAVES;

// GroupLanes with a weight beside every record: its records, its exchanges and its vote are reused as they are
template <int RPL>
struct WGroupLanes {
    cvxr::GroupLanes<RPL> g;
    WProb wp;
    double w[RPL > 0 ? RPL : 1];
    __device__ __forceinline__ void load()
    {
        if (RPL > 0) CVX_UNROLL for (int j = 0; j < RPL; ++j) {
            wrec_load(wp, g.lane + 16 * j, g.rec[j], w[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
        if (RPL > 0) {
            CVX_UNROLL for (int j = 0; j < RPL; ++j) {
                f(g.rec[j], w[j], (int64_t)(g.lane + 16 * j));
                __builtin_amdgcn_sched_barrier(0); // one record at a time (refine_lanes.h)
            }
        } else {
            const int n = wp.pb.n_p + wp.pb.n_l;
            for (int k = g.lane; k < n; k += 16) {
                Rec r;
                double wk;
                wrec_load(wp, k, r, wk);
                f(r, wk, (int64_t)k);
            }
        }
    }
    template <int N>
    __device__ __forceinline__ void sum(double *v) { g.template sum<N>(v); }
    __device__ __forceinline__ bool any(bool p) { return g.any(p); }
};

struct WBlockLanes {
    cvxr::BlockLanes b;
    WProb wp;
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
        const int n = wp.pb.n_p + wp.pb.n_l;
        for (int64_t k = threadIdx.x; k < n; k += TPB) { // (int64: k + TPB may pass 2^31)
            Rec r;
            double wk;
            wrec_load(wp, (int)k, r, wk);
            f(r, wk, k);
        }
    }
    template <int N>
    __device__ __forceinline__ void sum(double *v) { b.template sum<N>(v); }
    __device__ __forceinline__ bool any(bool p) { return b.any(p); }
};

struct Outputs {
    double *R, *t, *cost;           // [n][9], [n][3], [n][2]
    int32_t *iters, *status, *n_live, *n_inlier;
    double *rw_p, *rw_l;            // batch form: rw_p [n][n_p + n_l], rw_l unused; scenes: [n_pts], [n_lines]; optional
};

// The outputs of problem b as the writing lane addresses them, made BEFORE the loop.  Left as the kernel's uniform arguments, the six
// pointers are loaded at entry into scalar registers and live to the last line; the loop's constants then push them out into spills.
// The first N (in the order R, t, cost, iters, status, n_live) are moved to vector registers here -- the empty asm statement is the
// move: it emits nothing and tells the compiler that the value now lives in a vector register, so that it cannot be recomputed from
// the scalar argument later.  The rest stay uniform: each kernel takes what its two register files allow.
struct LaneOutputs {
    double *R, *t, *cost;
    int32_t *iters, *status, *n_live;
};

template <class T>
__device__ __forceinline__ T *in_vgpr(T *p)
{
    asm volatile("" : "+v"(p));
    return p;
}

template <int N>
__device__ __forceinline__ LaneOutputs lane_outputs(const Outputs &o, int64_t b)
{
    LaneOutputs l;
    l.R = o.R + 9 * b; l.t = o.t + 3 * b; l.cost = o.cost + 2 * b;
    l.iters = o.iters + b; l.status = o.status + b; l.n_live = o.n_live + b;
    if (N > 0) l.R = in_vgpr(l.R);
    if (N > 1) l.t = in_vgpr(l.t);
    if (N > 2) l.cost = in_vgpr(l.cost);
    if (N > 3) l.iters = in_vgpr(l.iters);
    if (N > 4) l.status = in_vgpr(l.status);
    if (N > 5) l.n_live = in_vgpr(l.n_live);
    return l;
}

// (a pose that was not refined passes through bit for bit: Rin / tin are read here, by the one lane that then writes -- they may alias the outputs)
template <bool COST_BEFORE> // (false: robust_problem has stored it)
__device__ __forceinline__ void write_result(const LaneOutputs &o, const Result &res, double cost_before, const double *Rin, const double *tin)
{
    const bool done = res.status <= cvxr::REFINE_MAXITER;
    CVX_UNROLL for (int i = 0; i < 9; ++i) o.R[i] = done ? res.R[i] : Rin[i];
    CVX_UNROLL for (int i = 0; i < 3; ++i) o.t[i] = done ? res.t[i] : tin[i];
    if (COST_BEFORE) o.cost[0] = cost_before;
    o.cost[1] = res.cost;
    *o.iters = res.iters; *o.status = res.status; *o.n_live = res.n_live;
}

struct BatchArgs {
    int64_t batch;
    int n_p, n_l, K_per_problem;
    uint32_t admit;
    int64_t status_stride;
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *wp, *wl;
    const int32_t *status;
    const uint8_t *mp, *ml;
    Opts opts;
    int loss_kind;   // the Loss is made from these two inside the kernel: computed there it lives in vector registers, passed whole it
    double scale_px; // crowds the scalar ones (the kernels' pointers already fill them)
    Outputs out;
};

// problem b of a batch form with weights: refine_view.h's batch_prob and the two weight slices (the per-record output is the caller's)
template <class A>
__device__ __forceinline__ const double *weighted_prob(const A &a, int64_t b, WProb &wp)
{
    const double *K = cvxr::batch_prob(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem, a.mp, a.ml, wp.pb);
    wp.wp = a.wp ? a.wp + b * a.n_p : nullptr;
    wp.wl = a.wl ? a.wl + b * a.n_l : nullptr;
    return K;
}

// problem b of this library's batch form: rho'(s_k) of its records goes to rw_p, the points' then the lines'
__device__ __forceinline__ const double *batch_prob(const BatchArgs &a, int64_t b, WProb &wp)
{
    const double *K = weighted_prob(a, b, wp);
    wp.ow_p = a.out.rw_p ? a.out.rw_p + b * ((int64_t)a.n_p + a.n_l) : nullptr;
    wp.ow_l = wp.ow_p ? wp.ow_p + a.n_p : nullptr;
    return K;
}

template <int RPL>
__global__ void __launch_bounds__(TPB) refine_robust_group_kernel(BatchArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    const bool mine = g < a.batch;
    const int64_t b = mine ? g : a.batch - 1; // an empty group of the last wavefront shadows the last problem and writes nothing
    WGroupLanes<RPL> ln;
    ln.g.lane = threadIdx.x & 15;
    const double *K = batch_prob(a, b, ln.wp);
    ln.load();
    const bool admit = mine && (!a.status || cvxr::admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.g.lane == 0;
    const LaneOutputs lo = lane_outputs<(RPL == 0 ? 1 : 0)>(a.out, b); // (the re-reading kernel's pointers crowd its scalar registers: it takes the cost before by value, the others have it stored)
    Result res;
    double c0;
    robust_problem(ln, K, a.R + 9 * b, a.t + 3 * b, admit, a.opts, make_loss(a.loss_kind, a.scale_px), res, c0, RPL > 0 && writer ? lo.cost : nullptr);
    if (writer) write_result<RPL == 0>(lo, res, c0, a.R + 9 * b, a.t + 3 * b);
}

// after refine_robust_group_kernel on the same stream: reads the refined poses and their statuses
__global__ void __launch_bounds__(TPB) robust_w_group_kernel(BatchArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return; // whole groups: the exchanges stay inside a group
    WGroupLanes<0> ln;
    ln.g.lane = threadIdx.x & 15;
    const double *K = batch_prob(a, g, ln.wp);
    const int n = robust_weights_problem(ln, ln.wp, K, a.out.R + 9 * g, a.out.t + 3 * g, a.out.status[g], make_loss(a.loss_kind, a.scale_px));
    if (ln.g.lane == 0) a.out.n_inlier[g] = n;
}

struct SceneArgs {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l; // [n_scenes + 1]; off_l may be null (no lines)
    const double *p2, *p3, *l2, *l3, *K, *R, *t, *wp, *wl;
    int K_per_scene;
    uint32_t admit;
    int64_t status_stride;
    const int32_t *status;
    const uint8_t *mp, *ml;       // [n_pts], [n_lines], optional
    Opts opts;
    int loss_kind;   // the Loss is made from these two inside the kernel: computed there it lives in vector registers, passed whole it
    double scale_px; // crowds the scalar ones (the kernels' pointers already fill them)
    Outputs out;
};

// the workgroup's scene with the weights: the poses R, t ([n_scenes][9] / [n_scenes][3]) staged in LDS with K and, behind them, the scale
// of the loss (a.scale_px, or a scale of the scene's own: refine_robust_auto_kernel.h)
__device__ __forceinline__ void scene_lanes(const SceneArgs &a, int64_t f, const double *R, const double *t, double scale, double *red, double *pose, WBlockLanes &ln)
{
    cvxr::stage_pose(a.K, a.K_per_scene, R, t, f, pose, [&] { if (threadIdx.x == POSE_N) pose[POSE_N] = scale; }); // (read back from LDS the loss is per-lane values too)
    const cvxn::Slice sp = cvxn::scene_slice(a.off_p, f, a.n_pts), sl = cvxr::line_slice(a.off_l, f, a.n_lines);
    ln.b.red = red;
    cvxr::scene_prob(sp, sl, a.p2, a.p3, a.l2, a.l3, a.mp, a.ml, ln.wp.pb);
    ln.wp.wp = in_vgpr(a.wp ? a.wp + sp.beg : nullptr); // (the scalar registers are full: see lane_outputs)
    ln.wp.wl = in_vgpr(a.wl ? a.wl + sl.beg : nullptr);
    ln.wp.ow_p = a.out.rw_p ? a.out.rw_p + sp.beg : nullptr;
    ln.wp.ow_l = a.out.rw_l ? a.out.rw_l + sl.beg : nullptr;
}

__global__ void __launch_bounds__(TPB) refine_robust_scenes_kernel(SceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[POSE_N + 1];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    WBlockLanes ln;
    scene_lanes(a, f, a.R, a.t, a.scale_px, red, pose, ln);
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    const LaneOutputs lo = lane_outputs<6>(a.out, f);
    Result res;
    double c0;
    const double *ps = pose;
    robust_problem(ln, ps, ps + 9, ps + 18, admit, a.opts, make_loss(a.loss_kind, ps[POSE_N]), res, c0);
    if (threadIdx.x == 0) write_result<true>(lo, res, c0, ps + 9, ps + 18);
}

// after refine_robust_scenes_kernel on the same stream
__global__ void __launch_bounds__(TPB) robust_w_scenes_kernel(SceneArgs a)
{
    __shared__ double red[(WAVES + 1) * ACC_N];
    __shared__ double pose[POSE_N + 1];
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    WBlockLanes ln;
    scene_lanes(a, f, a.out.R, a.out.t, a.scale_px, red, pose, ln);
    const double *ps = pose;
    const int n = robust_weights_problem(ln, ln.wp, ps, ps + 9, ps + 18, a.out.status[f], make_loss(a.loss_kind, ps[POSE_N]));
    if (threadIdx.x == 0) a.out.n_inlier[f] = n;
}

} // namespace cvxrb
