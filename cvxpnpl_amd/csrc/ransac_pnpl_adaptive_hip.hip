// ransac_pnpl_adaptive_hip.hip -- entry points of adaptive and guided RANSAC over points and lines
// (include/cvxpnpl_amd_ransac_pnpl_adaptive.h), built as libcvxpnpl_amd_ransac_pnpl_adaptive.so.  The kernels are
// ransac_pnpl_adaptive_kernel.h, the stopping rule ransac_adaptive_core.h, the pool rule ransac_guided_core.h.  Every entry point checks
// its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cvxpnpl_amd_ransac_pnpl_adaptive.h"
#include "ransac_pnpl_adaptive_kernel.h"

namespace {

thread_local char g_err[512] = "";

int set_err(const char *what, hipError_t e)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -2;
}

int bad(const char *who, const char *what)
{
    snprintf(g_err, sizeof(g_err), "%s: bad arguments (%s)", who, what);
    return -1;
}

// what the entry points of a round share: sizes, the active list, both offset arrays, both packed arrays.  Returns a message or null;
// fills the scene set.
const char *check_round(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *off_p, int64_t n_pts, const int64_t *off_l,
                        int64_t n_lines, const double *p2, const double *p3, const double *l2, const double *l3, cvxnl::SceneSet &s)
{
    if (n_scenes < 0 || n_active < 0 || n_pts < 0 || n_lines < 0) return "negative size";
    if (n_scenes > 0x7fffffffLL || n_active > 0x7fffffffLL) return "more scenes than an int32 index holds";
    if (n_scenes > 0 && n_active > 0) {
        if (!active) return "d_active is null";
        if (!off_p || !off_l) return "d_pt_offsets or d_ln_offsets is null";
        if (n_pts > 0 && (!p2 || !p3)) return "a point pointer is null";
        if (n_lines > 0 && (!l2 || !l3)) return "a line pointer is null";
    }
    s.n_scenes = n_scenes; s.n_pts = n_pts; s.n_lines = n_lines; s.off_p = off_p; s.off_l = off_l; s.p2 = p2; s.p3 = p3; s.l2 = l2; s.l3 = l3;
    s.K = nullptr; s.K_per_scene = 0;
    return nullptr;
}

const char *check_budget(int32_t hyp0, int32_t n_round, int32_t cap)
{
    if (hyp0 < 0 || n_round < 0 || cap < 0) return "negative hyp0, n_round or cap";
    if ((int64_t)hyp0 + n_round > (int64_t)cap) return "hyp0 + n_round exceeds cap";
    return nullptr;
}

bool bad_thresh(double thresh) { return !(thresh >= 0.0) || thresh > 1.7e308; }

constexpr int64_t GRID_Y = 65535; // active entries per launch of the two kernels whose grid is (hypotheses, entries)

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_err(what, e);
}

} // namespace

extern "C" const char *cvxpnpl_ransac_pnpl_adaptive_last_error(void) { return g_err; }

extern "C" int cvxpnpl_ransac_pnpl_adaptive_sample_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                            int32_t cap, int32_t pool_full, const int64_t *d_pt_offsets, int64_t n_pts,
                                                            const int64_t *d_ln_offsets, int64_t n_lines, const uint64_t *d_seeds,
                                                            const int32_t *d_order, const double *d_pts_2d, const double *d_pts_3d,
                                                            const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_scene,
                                                            int32_t *d_idx, double *d_Q45, double *d_B27, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_sample_assemble";
    cvxnla::SampleArgs a;
    if (const char *m = check_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad(who, m);
    if (pool_full < 0) return bad(who, "negative pool_full");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_seeds || !d_K || !d_Q45 || !d_B27) return bad(who, "d_seeds, d_K, d_Q45 or d_B27 is null");
    if (pool_full > 0 && !d_order) return bad(who, "d_order is null");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.hyp0 = hyp0; a.n_round = n_round; a.pool_full = pool_full;
    a.active = d_active; a.seed = d_seeds; a.order = d_order; a.idx = d_idx; a.Q45 = d_Q45; a.B27 = d_B27;
    const unsigned gx = (unsigned)(((int64_t)n_round + cvxnla::BLOCK - 1) / cvxnla::BLOCK);
    for (int64_t a0 = 0; a0 < n_active; a0 += GRID_Y) {
        a.act0 = a0;
        const int64_t ny = n_active - a0 < GRID_Y ? n_active - a0 : GRID_Y;
        hipLaunchKernelGGL(cvxnla::sample_assemble_active_kernel, dim3(gx, (unsigned)ny), dim3(cvxnla::BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("sample_assemble_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_adaptive_score(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t n_round,
                                                  const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                                  const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                                  const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                                  const double *d_line_2d, const double *d_line_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_score";
    cvxnla::ScoreArgs a;
    if (const char *m = check_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad(who, m);
    if (n_round < 0) return bad(who, "negative n_round");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad(who, "d_R, d_t, d_K or d_count is null");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.n_round = n_round; a.active = d_active; a.R = d_R; a.t = d_t;
    a.status = d_status; a.usable_mask = usable_mask; a.thresh = thresh; a.count = d_count;
    const unsigned gx = (unsigned)(((int64_t)n_round + cvxnla::BLOCK - 1) / cvxnla::BLOCK);
    for (int64_t a0 = 0; a0 < n_active; a0 += GRID_Y) {
        a.act0 = a0;
        const int64_t ny = n_active - a0 < GRID_Y ? n_active - a0 : GRID_Y;
        hipLaunchKernelGGL(cvxnla::score_pnpl_active_kernel, dim3(gx, (unsigned)ny), dim3(cvxnla::BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("score_pnpl_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_adaptive_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                   int32_t cap, double confidence, const int64_t *d_pt_offsets, int64_t n_pts,
                                                   const int64_t *d_ln_offsets, int64_t n_lines, const int32_t *d_count, const double *d_R,
                                                   const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                                   const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d, const double *d_line_3d,
                                                   double thresh, double *d_out_R, double *d_out_t, int32_t *d_head, int32_t *d_best,
                                                   uint8_t *d_mask_pts, uint8_t *d_mask_lines, int32_t *d_hyp_used, int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_adaptive_update";
    cvxnla::UpdateArgs a;
    if (const char *m = check_round(n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s))
        return bad(who, m);
    if (const char *m = check_budget(hyp0, n_round, cap)) return bad(who, m);
    if (cvxna::bad_confidence(confidence)) return bad(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (n_round < 1) return bad(who, "a round needs at least one hypothesis");
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || !d_best || !d_hyp_used || !d_done ||
        (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines))
        return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.hyp0 = hyp0; a.n_round = n_round; a.cap = cap; a.confidence = confidence;
    a.active = d_active; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t;
    a.head = d_head; a.best = d_best; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines; a.hyp_used = d_hyp_used; a.done = d_done;
    hipLaunchKernelGGL(cvxnla::update_pnpl_active_kernel, dim3((unsigned)n_active), dim3(cvxnla::BLOCK), 0, (hipStream_t)stream, a);
    return launched("update_pnpl_active_kernel launch");
}
