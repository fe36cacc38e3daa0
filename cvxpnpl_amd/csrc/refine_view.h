// refine_view.h -- where one problem's records, masks and pose are: the ONE statement of it for the five refinement libraries (DESIGN.md
// section 15).  No kernel.  batch_prob is host and device (the *_host entry points reach it through refine_entry.h's host_problem); the
// scene forms, whose offsets live on the device, are behind __HIPCC__.  Every function takes the FIELDS of an argument block, under the
// names all BatchArgs / VjpBatchArgs / SceneArgs / VjpSceneArgs share, and not the block: a kernel that never takes the address of its
// argument block reads it straight from the kernel-argument segment, and one reference to it -- into an inlined function too -- changes
// the code of the whole kernel.
#pragma once
#include <stdint.h>

#include "refine_core.h"
#if defined(__HIPCC__)
#include "ransac_common.h"
#endif

namespace cvxr {

// problem b of a batch form [B, n_p] + [B, n_l]: its records and masks into pb, its K returned (a pointer of a kind that has no records is
// never followed)
CVX_HD const double *batch_prob(int64_t b, int n_p, const double *p2, const double *p3, int n_l, const double *l2, const double *l3, const double *K,
                                int K_per_problem, const uint8_t *mp, const uint8_t *ml, Prob &pb)
{
    const cvx::ProblemView pv = cvx::make_view(b, n_p, p2, p3, n_l, l2, l3, K, K_per_problem);
    pb.n_p = n_p; pb.n_l = n_l;
    pb.p2 = pv.p2; pb.p3 = pv.p3; pb.l2 = pv.l2; pb.l3 = pv.l3;
    pb.mp = mp ? mp + b * n_p : nullptr;
    pb.ml = ml ? ml + b * n_l : nullptr;
    return pv.K;
}

#if defined(__HIPCC__)
// Scene f of a packed set.  Its slice of the lines, clamped to the array as cvxn::scene_slice clamps the points' (off_l null: no lines):
// the offsets live on the device, so that clamp and scene_prob's n_l are the only check they get.  A caller keeps both slices -- its
// weights, gradients and per-record outputs start at sp.beg / sl.beg too.
__device__ __forceinline__ cvxn::Slice line_slice(const int64_t *off_l, int64_t f, int64_t n_lines)
{
    cvxn::Slice sl{0, 0};
    if (off_l) sl = cvxn::scene_slice(off_l, f, n_lines);
    return sl;
}

// ... its records and masks into pb; n_p + n_l is kept within an int, which is how the lanes index a problem's records
__device__ __forceinline__ void scene_prob(cvxn::Slice sp, cvxn::Slice sl, const double *p2, const double *p3, const double *l2, const double *l3,
                                           const uint8_t *mp, const uint8_t *ml, Prob &pb)
{
    pb.n_p = sp.n;
    pb.n_l = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    pb.p2 = p2 + sp.beg * 2; pb.p3 = p3 + sp.beg * 3; // (never followed where the slice is empty)
    pb.l2 = l2 + sl.beg * 4; pb.l3 = l3 + sl.beg * 6;
    pb.mp = mp ? mp + sp.beg : nullptr;
    pb.ml = ml ? ml + sl.beg : nullptr;
}

// ... where its gradients go (G: cvxrg::Grads); an output that is not wanted stays null
template <class G>
__device__ __forceinline__ void scene_grads(cvxn::Slice sp, cvxn::Slice sl, double *g_p2, double *g_p3, double *g_l2, double *g_l3, G &g)
{
    g.p2 = g_p2 ? g_p2 + sp.beg * 2 : nullptr;
    g.p3 = g_p3 ? g_p3 + sp.beg * 3 : nullptr;
    g.l2 = g_l2 ? g_l2 + sl.beg * 4 : nullptr;
    g.l3 = g_l3 ? g_l3 + sl.beg * 6 : nullptr;
}

// ... and its K / R / t staged in LDS, pose[0 .. POSE_N), one element per thread, with the barrier after it (read from LDS they are
// per-lane values; read through a uniform pointer, the pose and everything computed from it would crowd the scalar registers).  R, t: the
// poses to stage, [n_scenes][9] / [n_scenes][3].  more(): what the threads from POSE_N on append behind the pose -- the upstream
// gradients (stage_upstream), a scale, nothing ([] {}) -- as further links of the one else-if chain, before the one barrier.
constexpr int POSE_N = 21, UPSTREAM_N = 12;

template <class F>
__device__ __forceinline__ void stage_pose(const double *K, int K_per_scene, const double *R, const double *t, int64_t f, double *pose, F more)
{
    if (threadIdx.x < 9) pose[threadIdx.x] = K[(K_per_scene ? f * 9 : 0) + threadIdx.x];
    else if (threadIdx.x < 18) pose[threadIdx.x] = R[9 * f + threadIdx.x - 9];
    else if (threadIdx.x < POSE_N) pose[threadIdx.x] = t[3 * f + threadIdx.x - 18];
    else more();
    __syncthreads();
}

// the links of that chain for the upstream gradients G_R, g_t of a backward pass (zeros where absent): pose[POSE_N .. POSE_N + UPSTREAM_N)
template <class F>
__device__ __forceinline__ void stage_upstream(const double *gR, const double *gt, int64_t f, double *pose, F more)
{
    if (threadIdx.x < POSE_N + 9) pose[threadIdx.x] = gR ? gR[9 * f + threadIdx.x - POSE_N] : 0.0;
    else if (threadIdx.x < POSE_N + UPSTREAM_N) pose[threadIdx.x] = gt ? gt[3 * f + threadIdx.x - POSE_N - 9] : 0.0;
    else more();
}
#endif // __HIPCC__

} // namespace cvxr
