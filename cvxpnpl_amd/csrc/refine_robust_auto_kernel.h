// refine_robust_auto_kernel.h -- the device side of include/cvxpnpl_amd_refine_robust_auto.h; the mathematics is
// refine_robust_auto_core.h, shared with the host path; the lanes, their exchanges and the argument blocks are refine_robust_kernel.h's
// and refine_lanes.h's.
//   robust_scale_group_kernel<RPL> / robust_scale_scenes_kernel     sigma per problem from the median of s_k.  16 lanes per problem with
//       1, 2 or 4 records (and their s_k, through all 63 rounds) in a lane's registers, RPL = 0 beyond 64 records: s_k is read again from
//       sq; one workgroup of 256 per scene, which reads sq again too.  A lane only ever reads back what it has written itself.
//   refine_robust_pp_group_kernel<RPL> / refine_robust_pp_scenes_kernel, robust_w_pp_group_kernel / robust_w_pp_scenes_kernel
//       refine_robust_kernel.h's kernels with the loss made from scale[b] (a null array: the uniform scale of the options).
//   robust_cov_group_kernel / robust_cov_scenes_kernel               the sandwich covariance at a pose, a pass of its own.
// All clamp what they index as refine_robust_kernel.h's do (through its batch_prob and scene_lanes, over refine_view.h); whole groups
// beyond the batch leave where no wavefront vote follows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine_robust_auto_core.h"
#include "refine_robust_kernel.h"
#include "refine_view.h"

namespace cvxra {

using cvxr::POSE_N;
using cvxr::TPB;
using cvxr::WAVES;

// refine_robust_kernel.h's argument blocks with what this library adds.  Of a.out the scale kernels use status, n_live and rw_p / rw_l
// (sq: where batch_prob and the scene's lanes put the per-record output); the covariance kernels use none of it.
struct AutoBatchArgs {
    cvxrb::BatchArgs a;
    const double *scale;      // [batch], null: a.scale_px (and null under l2)
    double *sigma, *med_sq;   // the scale kernels
    double *cov;              // the covariance kernels: [batch][36]
    int32_t *cov_status;
};

struct AutoSceneArgs {
    cvxrb::SceneArgs a;
    const double *scale;
    double *sigma, *med_sq;
    double *cov;
    int32_t *cov_status;
};

// ---- the lanes of scale_problem ----

template <int RPL>
struct SelGroupLanes {
    cvxrb::WGroupLanes<RPL> w;
    double v[RPL > 0 ? RPL : 1];
    __device__ __forceinline__ double &at(int k) { return k < w.wp.pb.n_p ? w.wp.ow_p[k] : w.wp.ow_l[k - w.wp.pb.n_p]; }
    template <class F>
    __device__ __forceinline__ void first(F f)
    {
        if (RPL > 0) {
            CVX_UNROLL for (int j = 0; j < RPL; ++j) {
                v[j] = f(w.g.rec[j], w.w[j]); // (a slot beyond the problem: kind 0, weight 0, the value -1 of a record that is not live)
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const int n = w.wp.pb.n_p + w.wp.pb.n_l;
            for (int k = w.g.lane; k < n; k += 16) {
                Rec r;
                double wk;
                cvxrb::wrec_load(w.wp, k, r, wk);
                at(k) = f(r, wk);
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void vals(F f)
    {
        if (RPL > 0) {
            CVX_UNROLL for (int j = 0; j < RPL; ++j) f(v[j]);
        } else {
            const int n = w.wp.pb.n_p + w.wp.pb.n_l;
            for (int k = w.g.lane; k < n; k += 16) f(at(k));
        }
    }
    __device__ __forceinline__ void finish(bool ok)
    {
        const int n = w.wp.pb.n_p + w.wp.pb.n_l;
        if (RPL > 0) {
            CVX_UNROLL for (int j = 0; j < RPL; ++j) {
                const int k = w.g.lane + 16 * j;
                if (k < n) at(k) = ok ? v[j] : NAN;
            }
        } else if (!ok) {
            for (int k = w.g.lane; k < n; k += 16) at(k) = NAN;
        }
    }
    template <int N>
    __device__ __forceinline__ void sum(double *x) { w.template sum<N>(x); }
};

struct SelBlockLanes {
    cvxrb::WBlockLanes w;
    __device__ __forceinline__ double &at(int k) { return k < w.wp.pb.n_p ? w.wp.ow_p[k] : w.wp.ow_l[k - w.wp.pb.n_p]; }
    template <class F>
    __device__ __forceinline__ void first(F f)
    {
        const int n = w.wp.pb.n_p + w.wp.pb.n_l;
        for (int64_t k = threadIdx.x; k < n; k += TPB) {
            Rec r;
            double wk;
            cvxrb::wrec_load(w.wp, (int)k, r, wk);
            at((int)k) = f(r, wk);
        }
    }
    template <class F>
    __device__ __forceinline__ void vals(F f)
    {
        const int n = w.wp.pb.n_p + w.wp.pb.n_l;
        for (int64_t k = threadIdx.x; k < n; k += TPB) f(at((int)k));
    }
    __device__ __forceinline__ void finish(bool ok)
    {
        const int n = w.wp.pb.n_p + w.wp.pb.n_l;
        if (!ok) for (int64_t k = threadIdx.x; k < n; k += TPB) at((int)k) = NAN;
    }
    template <int N>
    __device__ __forceinline__ void sum(double *x) { w.template sum<N>(x); }
};

// ---- 1. the scale ----

template <int RPL>
__global__ void __launch_bounds__(TPB) robust_scale_group_kernel(AutoBatchArgs pa)
{
    const cvxrb::BatchArgs &a = pa.a;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return; // whole groups: the exchanges stay inside a group
    SelGroupLanes<RPL> sl;
    sl.w.g.lane = threadIdx.x & 15;
    const double *K = cvxrb::batch_prob(a, g, sl.w.wp);
    sl.w.load();
    const bool admit = !a.status || cvxr::admitted(a.status[g * a.status_stride], a.admit);
    ScaleResult res;
    scale_problem(sl, K, a.R + 9 * g, a.t + 3 * g, admit, res);
    if (sl.w.g.lane == 0) {
        pa.sigma[g] = res.sigma; pa.med_sq[g] = res.med_sq;
        a.out.n_live[g] = res.n_live; a.out.status[g] = res.status;
    }
}

__global__ void __launch_bounds__(TPB) robust_scale_scenes_kernel(AutoSceneArgs pa)
{
    __shared__ double red[(WAVES + 1) * cvxr::ACC_N];
    __shared__ double pose[POSE_N + 1];
    const cvxrb::SceneArgs &a = pa.a;
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    SelBlockLanes sl;
    cvxrb::scene_lanes(a, f, a.R, a.t, 0.0, red, pose, sl.w);
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    const double *ps = pose;
    ScaleResult res;
    scale_problem(sl, ps, ps + 9, ps + 18, admit, res);
    if (threadIdx.x == 0) {
        pa.sigma[f] = res.sigma; pa.med_sq[f] = res.med_sq;
        a.out.n_live[f] = res.n_live; a.out.status[f] = res.status;
    }
}

// ---- 2. the loop at a scale per problem: refine_robust_kernel.h's kernels with scale[b] ----

template <int RPL>
__global__ void __launch_bounds__(TPB) refine_robust_pp_group_kernel(AutoBatchArgs pa)
{
    const cvxrb::BatchArgs &a = pa.a;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    const bool mine = g < a.batch;
    const int64_t b = mine ? g : a.batch - 1; // an empty group of the last wavefront shadows the last problem and writes nothing
    PerProblemScale<cvxrb::WGroupLanes<RPL>> ln;
    ln.g.lane = threadIdx.x & 15;
    const double *K = cvxrb::batch_prob(a, b, ln.wp);
    ln.load();
    const double scale = pa.scale ? pa.scale[b] : a.scale_px;
    ln.bad_scale = !scale_usable(a.loss_kind, scale);
    const bool admit = mine && (!a.status || cvxr::admitted(a.status[b * a.status_stride], a.admit));
    const bool writer = mine && ln.g.lane == 0;
    const cvxrb::LaneOutputs lo = cvxrb::lane_outputs<(RPL == 0 ? 1 : 0)>(a.out, b);
    cvxrb::Result res;
    double c0;
    cvxrb::robust_problem(ln, K, a.R + 9 * b, a.t + 3 * b, admit, a.opts, cvxrb::make_loss(a.loss_kind, scale), res, c0, RPL > 0 && writer ? lo.cost : nullptr);
    if (writer) cvxrb::write_result<RPL == 0>(lo, res, c0, a.R + 9 * b, a.t + 3 * b);
}

// after refine_robust_pp_group_kernel on the same stream: reads the refined poses and their statuses
__global__ void __launch_bounds__(TPB) robust_w_pp_group_kernel(AutoBatchArgs pa)
{
    const cvxrb::BatchArgs &a = pa.a;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return;
    cvxrb::WGroupLanes<0> ln;
    ln.g.lane = threadIdx.x & 15;
    const double *K = cvxrb::batch_prob(a, g, ln.wp);
    const double scale = pa.scale ? pa.scale[g] : a.scale_px;
    const int n = cvxrb::robust_weights_problem(ln, ln.wp, K, a.out.R + 9 * g, a.out.t + 3 * g, a.out.status[g], cvxrb::make_loss(a.loss_kind, scale));
    if (ln.g.lane == 0) a.out.n_inlier[g] = n;
}

__global__ void __launch_bounds__(TPB) refine_robust_pp_scenes_kernel(AutoSceneArgs pa)
{
    __shared__ double red[(WAVES + 1) * cvxr::ACC_N];
    __shared__ double pose[POSE_N + 1];
    const cvxrb::SceneArgs &a = pa.a;
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return; // (workgroup-uniform)
    PerProblemScale<cvxrb::WBlockLanes> ln;
    cvxrb::scene_lanes(a, f, a.R, a.t, pa.scale ? pa.scale[f] : a.scale_px, red, pose, ln);
    const bool admit = !a.status || cvxr::admitted(a.status[f * a.status_stride], a.admit);
    const cvxrb::LaneOutputs lo = cvxrb::lane_outputs<6>(a.out, f);
    cvxrb::Result res;
    double c0;
    const double *ps = pose;
    ln.bad_scale = !scale_usable(a.loss_kind, ps[POSE_N]);
    cvxrb::robust_problem(ln, ps, ps + 9, ps + 18, admit, a.opts, cvxrb::make_loss(a.loss_kind, ps[POSE_N]), res, c0);
    if (threadIdx.x == 0) cvxrb::write_result<true>(lo, res, c0, ps + 9, ps + 18);
}

__global__ void __launch_bounds__(TPB) robust_w_pp_scenes_kernel(AutoSceneArgs pa)
{
    __shared__ double red[(WAVES + 1) * cvxr::ACC_N];
    __shared__ double pose[POSE_N + 1];
    const cvxrb::SceneArgs &a = pa.a;
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    cvxrb::WBlockLanes ln;
    cvxrb::scene_lanes(a, f, a.out.R, a.out.t, pa.scale ? pa.scale[f] : a.scale_px, red, pose, ln);
    const double *ps = pose;
    const int n = cvxrb::robust_weights_problem(ln, ln.wp, ps, ps + 9, ps + 18, a.out.status[f], cvxrb::make_loss(a.loss_kind, ps[POSE_N]));
    if (threadIdx.x == 0) a.out.n_inlier[f] = n;
}

// ---- 3. the sandwich covariance ----

// (a.status: the refinement's status of the pose, optional; a pose whose status is not 0 or 1 is not differentiated)
__device__ __forceinline__ bool differentiated(const int32_t *status, int64_t i)
{
    if (!status) return true;
    const int32_t s = status[i];
    return s == cvxr::REFINE_CONVERGED || s == cvxr::REFINE_MAXITER;
}

__global__ void __launch_bounds__(TPB) robust_cov_group_kernel(AutoBatchArgs pa)
{
    const cvxrb::BatchArgs &a = pa.a;
    const int64_t g = (int64_t)blockIdx.x * (TPB / 16) + (threadIdx.x >> 4);
    if (g >= a.batch) return;
    cvxrb::WGroupLanes<0> ln;
    ln.g.lane = threadIdx.x & 15;
    const double *K = cvxrb::batch_prob(a, g, ln.wp);
    const double scale = pa.scale ? pa.scale[g] : a.scale_px;
    const bool usable = scale_usable(a.loss_kind, scale);
    const int st = robust_cov_problem(ln, K, a.R + 9 * g, a.t + 3 * g, differentiated(a.status, g), !usable, cvxrb::make_loss(a.loss_kind, usable ? scale : 1.0),
                                      ln.g.lane == 0 ? pa.cov + 36 * g : nullptr);
    if (ln.g.lane == 0) pa.cov_status[g] = st;
}

__global__ void __launch_bounds__(TPB) robust_cov_scenes_kernel(AutoSceneArgs pa)
{
    __shared__ double red[(WAVES + 1) * cvxr::ACC_N];
    __shared__ double pose[POSE_N + 1];
    const cvxrb::SceneArgs &a = pa.a;
    const int64_t f = blockIdx.x;
    if (f >= a.n_scenes) return;
    cvxrb::WBlockLanes ln;
    cvxrb::scene_lanes(a, f, a.R, a.t, pa.scale ? pa.scale[f] : a.scale_px, red, pose, ln);
    const double *ps = pose;
    const bool usable = scale_usable(a.loss_kind, ps[POSE_N]);
    const int st = robust_cov_problem(ln, ps, ps + 9, ps + 18, differentiated(a.status, f), !usable, cvxrb::make_loss(a.loss_kind, usable ? ps[POSE_N] : 1.0),
                                      threadIdx.x == 0 ? pa.cov + 36 * f : nullptr);
    if (threadIdx.x == 0) pa.cov_status[f] = st;
}

} // namespace cvxra
