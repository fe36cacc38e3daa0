// ransac_hip.hip -- entry points of RANSAC over many scenes (include/cvxpnpl_amd_ransac.h), built as libcvxpnpl_amd_ransac.so.
// The kernels are ransac_kernel.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cvxpnpl_amd_ransac.h"
#include "ransac_kernel.h"

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

// what every entry point shares: sizes, the offsets, the packed scene.  Returns a message or null.
const char *check_scenes(int64_t n_scenes, const int64_t *off, int64_t n_total, const double *s2, const double *s3)
{
    if (n_scenes < 0 || n_total < 0) return "negative size";
    if (n_scenes == 0) return nullptr;
    if (!off) return "d_offsets is null";
    if (n_total > 0 && (!s2 || !s3)) return "a scene pointer is null";
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

extern "C" const char *cvxpnpl_ransac_last_error(void) { return g_err; }

extern "C" int cvxpnpl_ransac_sample_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const uint64_t *d_seeds,
                                            const double *d_scene_2d, const double *d_scene_3d, const double *d_K, int32_t *d_idx, double *d_pts_2d,
                                            double *d_pts_3d, double *d_K_hyp, void *stream)
{
    const char *who = "cvxpnpl_ransac_sample_scenes";
    if (const char *m = check_scenes(n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad(who, m);
    if (n_hyp < 0) return bad(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_seeds || !d_pts_2d || !d_pts_3d) return bad(who, "d_seeds, d_pts_2d or d_pts_3d is null");
    if ((d_K == nullptr) != (d_K_hyp == nullptr)) return bad(who, "d_K and d_K_hyp go together");
    cvxn::SampleScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.seed = d_seeds; a.s2 = d_scene_2d; a.s3 = d_scene_3d;
    a.K = d_K; a.idx = d_idx; a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.Kh = d_K_hyp;
    const unsigned gx = (unsigned)(((int64_t)n_hyp + cvxn::SCENE_BLOCK - 1) / cvxn::SCENE_BLOCK);
    for (int64_t f0 = 0; f0 < n_scenes; f0 += GRID_Y) {
        a.scene0 = f0;
        const int64_t ny = n_scenes - f0 < GRID_Y ? n_scenes - f0 : GRID_Y;
        hipLaunchKernelGGL(cvxn::sample_scenes_kernel, dim3(gx, (unsigned)ny), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("sample_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_score_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const double *d_R,
                                           const double *d_t, const int32_t *d_status, uint32_t usable_mask, const double *d_K, int32_t K_per_scene,
                                           const double *d_scene_2d, const double *d_scene_3d, double thresh, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_score_scenes";
    if (const char *m = check_scenes(n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad(who, m);
    if (n_hyp < 0) return bad(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (!d_R || !d_t || !d_K || !d_count) return bad(who, "d_R, d_t, d_K or d_count is null");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    cvxn::ScoreScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.R = d_R; a.t = d_t; a.status = d_status;
    a.usable_mask = usable_mask; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.count = d_count;
    const unsigned gx = (unsigned)(((int64_t)n_hyp + cvxn::SCENE_BLOCK - 1) / cvxn::SCENE_BLOCK);
    for (int64_t f0 = 0; f0 < n_scenes; f0 += GRID_Y) {
        a.scene0 = f0;
        const int64_t ny = n_scenes - f0 < GRID_Y ? n_scenes - f0 : GRID_Y;
        hipLaunchKernelGGL(cvxn::score_scenes_kernel, dim3(gx, (unsigned)ny), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    }
    return launched("score_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_select_scenes(int64_t n_scenes, int32_t n_hyp, const int64_t *d_offsets, int64_t n_total, const int32_t *d_count,
                                            const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K, int32_t K_per_scene,
                                            const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_out_R, double *d_out_t,
                                            int32_t *d_head, uint8_t *d_mask, void *stream)
{
    const char *who = "cvxpnpl_ransac_select_scenes";
    if (const char *m = check_scenes(n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_hyp < 1) return bad(who, "a scene needs at least one hypothesis");
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head || (n_total > 0 && !d_mask)) return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    cvxn::SelectScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.off = d_offsets; a.count = d_count; a.R = d_R; a.t = d_t; a.status = d_status;
    a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.out_R = d_out_R; a.out_t = d_out_t;
    a.head = d_head; a.mask = d_mask;
    hipLaunchKernelGGL(cvxn::select_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_scenes_kernel launch");
}

extern "C" int cvxpnpl_ransac_assemble_consensus(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_scene_2d,
                                                 const double *d_scene_3d, const uint8_t *d_mask, const double *d_K, int32_t K_per_scene,
                                                 double *d_B27, double *d_Q45, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_assemble_consensus";
    if (const char *m = check_scenes(n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_K || !d_B27 || !d_Q45 || !d_count || (n_total > 0 && !d_mask)) return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    cvxn::ConsensusArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.off = d_offsets; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.mask = d_mask; a.K = d_K;
    a.K_per_scene = K_per_scene; a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxn::assemble_consensus_kernel, dim3((unsigned)n_scenes), dim3(64), 0, (hipStream_t)stream, a);
    return launched("assemble_consensus_kernel launch");
}

extern "C" int cvxpnpl_ransac_refit_update_scenes(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, const double *d_fit_R,
                                                  const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count, const double *d_K,
                                                  int32_t K_per_scene, const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_R,
                                                  double *d_t, int32_t *d_head, uint8_t *d_mask, void *stream)
{
    const char *who = "cvxpnpl_ransac_refit_update_scenes";
    if (const char *m = check_scenes(n_scenes, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad(who, m);
    if (n_scenes == 0) return 0;
    if (n_scenes > 0x7fffffffLL) return bad(who, "more scenes than one launch holds");
    if (!d_fit_R || !d_fit_t || !d_fit_status || !d_fit_count || !d_K || !d_R || !d_t || !d_head || (n_total > 0 && !d_mask)) return bad(who, "a null pointer");
    if (K_per_scene != 0 && K_per_scene != 1) return bad(who, "K_per_scene is 0 or 1");
    if (bad_thresh(thresh)) return bad(who, "thresh is not a finite non-negative number");
    cvxn::RefitScenesArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.off = d_offsets; a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status;
    a.fit_cnt = d_fit_count; a.K = d_K; a.K_per_scene = K_per_scene; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.io_R = d_R;
    a.io_t = d_t; a.head = d_head; a.mask = d_mask;
    hipLaunchKernelGGL(cvxn::refit_update_scenes_kernel, dim3((unsigned)n_scenes), dim3(cvxn::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("refit_update_scenes_kernel launch");
}
