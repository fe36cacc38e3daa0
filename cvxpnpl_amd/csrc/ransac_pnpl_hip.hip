// ransac_pnpl_hip.hip -- entry points of RANSAC over points and lines, many scenes (include/cvxpnpl_amd_ransac_pnpl.h), built as
// libcvxpnpl_amd_ransac_pnpl.so.  The kernels are ransac_pnpl_kernel.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cvxpnpl_amd_ransac_pnpl.h"
#include "ransac_pnpl_kernel.h"

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

// what every entry point shares: sizes, both offset arrays, both packed arrays, K.  Returns a message or null; fills the scene set.
const char *check_scenes(int64_t n_scenes, const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines, const double *p2, const double *p3,
                         const double *l2, const double *l3, cvxnl::SceneSet &s)
{
    if (n_scenes < 0 || n_pts < 0 || n_lines < 0) return "negative size";
    if (n_scenes > 0) {
        if (!off_p || !off_l) return "d_pt_offsets or d_ln_offsets is null";
        if (n_pts > 0 && (!p2 || !p3)) return "a point pointer is null";
        if (n_lines > 0 && (!l2 || !l3)) return "a line pointer is null";
    }
    s.n_scenes = n_scenes; s.n_pts = n_pts; s.n_lines = n_lines; s.off_p = off_p; s.off_l = off_l; s.p2 = p2; s.p3 = p3; s.l2 = l2; s.l3 = l3;
    s.K = nullptr; s.K_per_scene = 0;
    return nullptr;
}

bool bad_thresh(double thresh) { return !(thresh >= 0.0) || thresh > 1.7e308; }

constexpr int64_t GRID_Y = 65535; // scenes per launch of the two kernels whose grid is (hypotheses, scenes)

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_err(what, e);
}

} // namespace

extern "C" const char *cvxpnpl_ransac_pnpl_last_error(void) { return g_err; }

extern "C" int cvxpnpl_ransac_pnpl_sample_assemble(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                                   int64_t n_lines, const uint64_t *d_seeds, const double *d_pts_2d, const double *d_pts_3d,
                                                   const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_scene, int32_t *d_idx,
                                                   double *d_Q45, double *d_B27, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_sample_assemble";
    cvxnl::SampleArgs a;
    if (const char *m = check_scenes(n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad(who, m);
    if (n_hyp < 0) return bad(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_seeds || !d_K || !d_Q45 || !d_B27) return bad(who, "d_seeds, d_K, d_Q45 or d_B27 is null");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.seed = d_seeds; a.idx = d_idx; a.Q45 = d_Q45; a.B27 = d_B27;
    const unsigned gx = (unsigned)(((int64_t)n_hyp + cvxnl::BLOCK - 1) / cvxnl::BLOCK);
    for (int64_t f0 = 0; f0 < n_scenes; f0 += GRID_Y) {
        a.scene0 = f0;
        const int64_t ny = n_scenes - f0 < GRID_Y ? n_scenes - f0 : GRID_Y;
        hipLaunchKernelGGL(cvxnl::sample_assemble_kernel, dim3(gx, (unsigned)ny), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("sample_assemble_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_score(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                         int64_t n_lines, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                                         const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                         const double *d_line_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_score";
    cvxnl::ScoreArgs a;
    if (const char *m = check_scenes(n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad(who, m);
    if (n_hyp < 0) return bad(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad(who, "d_R, d_t, d_K or d_count is null");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.R = d_R; a.t = d_t; a.status = d_status; a.usable_mask = usable_mask;
    a.thresh = thresh; a.count = d_count;
    const unsigned gx = (unsigned)(((int64_t)n_hyp + cvxnl::BLOCK - 1) / cvxnl::BLOCK);
    for (int64_t f0 = 0; f0 < n_scenes; f0 += GRID_Y) {
        a.scene0 = f0;
        const int64_t ny = n_scenes - f0 < GRID_Y ? n_scenes - f0 : GRID_Y;
        hipLaunchKernelGGL(cvxnl::score_kernel, dim3(gx, (unsigned)ny), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("score_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_select(int64_t n_scenes, int32_t n_hyp, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                          int64_t n_lines, const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status,
                                          const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                          const double *d_line_3d, double thresh, double *d_out_R, double *d_out_t, int32_t *d_head, uint8_t *d_mask_pts,
                                          uint8_t *d_mask_lines, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_select";
    cvxnl::SelectArgs a;
    if (const char *m = check_scenes(n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_hyp < 1) return bad(who, "a scene needs at least one hypothesis");
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines))
        return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_hyp = n_hyp; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status; a.thresh = thresh;
    a.out_R = d_out_R; a.out_t = d_out_t; a.head = d_head; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines;
    hipLaunchKernelGGL(cvxnl::select_kernel, dim3((unsigned)n_scenes), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_assemble_consensus(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets,
                                                      int64_t n_lines, const double *d_pts_2d, const double *d_pts_3d, const double *d_line_2d,
                                                      const double *d_line_3d, const uint8_t *d_mask_pts, const uint8_t *d_mask_lines, const double *d_K,
                                                      int32_t K_per_scene, double *d_B27, double *d_Q45, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_assemble_consensus";
    cvxnl::ConsensusArgs a;
    if (const char *m = check_scenes(n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_K || !d_B27 || !d_Q45 || !d_count || (n_pts > 0 && !d_mask_pts) || (n_lines > 0 && !d_mask_lines)) return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines; a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxnl::assemble_consensus_kernel, dim3((unsigned)n_scenes), dim3(64), 0, (hipStream_t)stream, a);
    return launched("assemble_consensus_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_refit_update(int64_t n_scenes, const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                                const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count,
                                                const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                                const double *d_line_2d, const double *d_line_3d, double thresh, double *d_R, double *d_t, int32_t *d_head,
                                                uint8_t *d_mask_pts, uint8_t *d_mask_lines, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_refit_update";
    cvxnl::RefitArgs a;
    if (const char *m = check_scenes(n_scenes, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d, d_line_3d, a.s)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_fit_R || !d_fit_t || !d_fit_status || !d_fit_count || !d_K || !d_R || !d_t || !d_head || (n_pts > 0 && !d_mask_pts) ||
        (n_lines > 0 && !d_mask_lines))
        return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status; a.fit_cnt = d_fit_count;
    a.thresh = thresh; a.io_R = d_R; a.io_t = d_t; a.head = d_head; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines;
    hipLaunchKernelGGL(cvxnl::refit_update_kernel, dim3((unsigned)n_scenes), dim3(cvxnl::BLOCK), 0, (hipStream_t)stream, a);
    return launched("refit_update_kernel launch");
}
