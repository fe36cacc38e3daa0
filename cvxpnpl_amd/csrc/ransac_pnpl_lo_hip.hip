// ransac_pnpl_lo_hip.hip -- entry points of local optimisation in adaptive RANSAC over points and lines
// (include/cvxpnpl_amd_ransac_pnpl_lo.h), built as libcvxpnpl_amd_ransac_pnpl_lo.so.  The kernels are ransac_pnpl_lo_kernel.h, the rules
// ransac_pnpl_lo_core.h and ransac_lo_core.h, the shared checks ransac_entry.h.  Every entry point checks its arguments before it launches
// anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_pnpl_lo.h"
#include "host_pool.h"
#include "ransac_entry.h"
#include "ransac_pnpl_lo_kernel.h"

using namespace cvxne;

namespace {

// The sizes of a round and -- a call that does something -- its active list and scene set, every pointer under its own name (pre: "d_"
// for a device entry point, "" for the host's); fills s, K left to the entry point.
int check_round_named(const char *who, const char *pre, int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *off_p, int64_t n_pts,
                      const int64_t *off_l, int64_t n_lines, const double *p2, const double *p3, const double *l2, const double *l3, cvxnl::SceneSet &s)
{
    if (const char *m = check_sizes(true, n_scenes, n_active, n_pts, n_lines)) return bad_args(who, m);
    fill_scene_set(s, n_scenes, off_p, n_pts, off_l, n_lines, p2, p3, l2, l3);
    if (n_scenes == 0 || n_active == 0) return 0;
    const void *none = who; // (a half without records may be null)
    const Named scene[] = {{"active", active}, {"pt_offsets", off_p}, {"ln_offsets", off_l}, {"pts_2d", n_pts > 0 ? p2 : none}, {"pts_3d", n_pts > 0 ? p3 : none},
                           {"line_2d", n_lines > 0 ? l2 : none}, {"line_3d", n_lines > 0 ? l3 : none}};
    for (const Named &n : scene)
        if (!n.p) return cvxee::fail(-1, "%s: bad arguments (%s%s is null)", who, pre, n.name);
    return 0;
}

// one entry of the host assembly: the first-three scans and the lanes of lo_assemble_pnpl_active_kernel, the rest cvxas::assemble_entry
void host_entry(int64_t ai, int64_t f, const cvxnl::SceneSet &s, const double *R, const double *t, double th, double *B27, double *Q45, int32_t *count)
{
    using namespace cvxnllo;
    const cvxnl::Scene sc = scene(s, f);
    double Ki[9], det;
    cvx::inv3(sc.K, Ki, det);
    cvxn::Camera cam;
    cvxnlo::camera(R + f * 9, t + f * 3, sc.K, cam);
    const double th2 = th * th;
    int fp[3] = {0, 0, 0}, fl[3] = {0, 0, 0}, nfp = 0, nfl = 0;
    for (int64_t m = 0; m < sc.P && nfp < 3; ++m)
        if (cvxnlo::taken(cam, sc.p2, sc.p3, m, th2)) fp[nfp++] = (int)m;
    const int want = cvxas::centre_lines_wanted(nfp);
    for (int64_t m = 0; m < sc.L && nfl < want; ++m)
        if (line_taken(cam, sc.l2, sc.l3, m, th)) fl[nfl++] = (int)m;
    double c[3];
    cvxas::centre(nfp, fp, nfl, fl, sc.p3, sc.l3, c);
    cvxas::assemble_entry(ai, c, det, [&](int l, cvx::Gram &g) { return lane_sums(l, sc, cam, th, th2, Ki, c, g); }, B27, Q45, count);
}

} // namespace

extern "C" const char *cvxpnpl_ransac_pnpl_lo_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_pnpl_lo_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, const int64_t *d_pt_offsets, int64_t n_pts,
                                               const int64_t *d_ln_offsets, int64_t n_lines, const double *d_pts_2d, const double *d_pts_3d,
                                               const double *d_line_2d, const double *d_line_3d, const double *d_R, const double *d_t,
                                               const double *d_K, int32_t K_per_scene, double thresh_k, double *d_B27, double *d_Q45,
                                               int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_lo_assemble";
    cvxnllo::LoAssembleArgs a;
    if (int rc = check_round_named(who, "d_", n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d,
                                   d_line_3d, a.s))
        return rc;
    if (n_scenes == 0 || n_active == 0) return 0;
    if (int rc = null_among(who, {{"d_R", d_R}, {"d_t", d_t}, {"d_K", d_K}, {"d_B27", d_B27}, {"d_Q45", d_Q45}, {"d_count", d_count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh_k)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.active = d_active; a.R = d_R; a.t = d_t; a.thresh_k = thresh_k;
    a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxnllo::lo_assemble_pnpl_active_kernel, dim3((unsigned)n_active), dim3(cvxnllo::LANES), 0, (hipStream_t)stream, a);
    return launched("lo_assemble_pnpl_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_lo_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t cap, double confidence,
                                             const int64_t *d_pt_offsets, int64_t n_pts, const int64_t *d_ln_offsets, int64_t n_lines,
                                             const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count,
                                             const double *d_K, int32_t K_per_scene, const double *d_pts_2d, const double *d_pts_3d,
                                             const double *d_line_2d, const double *d_line_3d, double thresh, double *d_io_R, double *d_io_t,
                                             int32_t *d_head, int32_t *d_best, uint8_t *d_mask_pts, uint8_t *d_mask_lines, const int32_t *d_hyp_used,
                                             int32_t *d_lo_taken, int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_pnpl_lo_update";
    cvxnllo::LoUpdateArgs a;
    if (int rc = check_round_named(who, "d_", n_scenes, n_active, d_active, d_pt_offsets, n_pts, d_ln_offsets, n_lines, d_pts_2d, d_pts_3d, d_line_2d,
                                   d_line_3d, a.s))
        return rc;
    if (cap < 0) return bad_args(who, "negative cap");
    if (cvxna::bad_confidence(confidence)) return bad_args(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (int rc = null_among(who, {{"d_fit_R", d_fit_R}, {"d_fit_t", d_fit_t}, {"d_fit_status", d_fit_status}, {"d_fit_count", d_fit_count}, {"d_K", d_K},
                                  {"d_io_R", d_io_R}, {"d_io_t", d_io_t}, {"d_head", d_head}, {"d_best", d_best}, {"d_hyp_used", d_hyp_used},
                                  {"d_lo_taken", d_lo_taken}, {"d_done", d_done}}))
        return rc;
    if (n_pts > 0 && !d_mask_pts) return bad_args(who, "d_mask_pts is null");
    if (n_lines > 0 && !d_mask_lines) return bad_args(who, "d_mask_lines is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    a.s.K = d_K; a.s.K_per_scene = K_per_scene; a.n_active = n_active; a.cap = cap; a.confidence = confidence; a.active = d_active;
    a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status; a.fit_cnt = d_fit_count; a.thresh = thresh; a.io_R = d_io_R; a.io_t = d_io_t;
    a.head = d_head; a.best = d_best; a.mask_p = d_mask_pts; a.mask_l = d_mask_lines; a.hyp_used = d_hyp_used; a.lo_taken = d_lo_taken; a.done = d_done;
    hipLaunchKernelGGL(cvxnllo::lo_update_pnpl_active_kernel, dim3((unsigned)n_active), dim3(cvxnllo::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("lo_update_pnpl_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_pnpl_lo_assemble_host(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *pt_offsets, int64_t n_pts,
                                                    const int64_t *ln_offsets, int64_t n_lines, const double *pts_2d, const double *pts_3d,
                                                    const double *line_2d, const double *line_3d, const double *R, const double *t, const double *K,
                                                    int32_t K_per_scene, double thresh_k, double *B27, double *Q45, int32_t *count, int32_t n_threads)
{
    const char *who = "cvxpnpl_ransac_pnpl_lo_assemble_host";
    cvxnl::SceneSet s;
    if (int rc = check_round_named(who, "", n_scenes, n_active, active, pt_offsets, n_pts, ln_offsets, n_lines, pts_2d, pts_3d, line_2d, line_3d, s)) return rc;
    if (n_scenes == 0 || n_active == 0) return 0;
    if (int rc = null_among(who, {{"R", R}, {"t", t}, {"K", K}, {"B27", B27}, {"Q45", Q45}, {"count", count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh_k)) return bad_args(who, m);
    s.K = K; s.K_per_scene = K_per_scene;
    cvxh::for_chunks(n_active, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t ai = lo; ai < hi; ++ai) { // the kernel's workgroup
            const int64_t f = active[ai];
            if (f < 0 || f >= n_scenes) continue; // skipped, not clamped
            host_entry(ai, f, s, R, t, thresh_k, B27, Q45, count);
        }
    });
    return 0;
}
