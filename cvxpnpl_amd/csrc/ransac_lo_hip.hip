// ransac_lo_hip.hip -- entry points of local optimisation in adaptive RANSAC (include/cvxpnpl_amd_ransac_lo.h), built as
// libcvxpnpl_amd_ransac_lo.so.  The kernels are ransac_lo_kernel.h, the rules ransac_lo_core.h and ransac_assemble_core.h, the shared checks
// ransac_entry.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_lo.h"
#include "host_pool.h"
#include "ransac_entry.h"
#include "ransac_lo_kernel.h"

using namespace cvxne;

namespace {

// one entry of the host assembly: the first-three scan and the lanes of lo_assemble_active_kernel, the rest cvxas::assemble_entry
void host_entry(int64_t ai, int64_t f, const int64_t *off, int64_t n_total, const double *scene_2d, const double *scene_3d, const double *R,
                const double *t, const double *K, int32_t K_per_scene, double th2, double *B27, double *Q45, int32_t *count)
{
    using namespace cvxnlo;
    const cvxn::Slice sl = cvxn::scene_slice(off, f, n_total);
    const double *s2 = scene_2d + sl.beg * 2, *s3 = scene_3d + sl.beg * 3;
    const double *Kc = K + (K_per_scene ? f * 9 : 0);
    double Ki[9], det;
    cvx::inv3(Kc, Ki, det);
    cvxn::Camera cam;
    camera(R + f * 9, t + f * 3, Kc, cam);
    int first[3] = {0, 0, 0}, nf = 0;
    for (int m = 0; m < sl.n && nf < 3; ++m)
        if (taken(cam, s2, s3, m, th2)) first[nf++] = m;
    double c[3];
    cvxas::centre(nf, first, s3, c);
    cvxas::assemble_entry(ai, c, det, [&](int l, cvx::Gram &g) { return lane_sums(l, sl.n, s2, s3, cam, th2, Ki, c, g); }, B27, Q45, count);
}

} // namespace

extern "C" const char *cvxpnpl_ransac_lo_last_error(void) { return err_buf(); }

extern "C" int cvxpnpl_ransac_lo_init(int64_t n_scenes, int32_t *d_lo_taken, void *stream)
{
    const char *who = "cvxpnpl_ransac_lo_init";
    if (const char *m = check_sizes(true, n_scenes, 0, 0)) return bad_args(who, m);
    if (n_scenes == 0) return 0;
    if (!d_lo_taken) return bad_args(who, "d_lo_taken is null");
    cvxnlo::LoInitArgs a;
    a.n_scenes = n_scenes; a.lo_taken = d_lo_taken;
    hipLaunchKernelGGL(cvxnlo::lo_init_kernel, dim3(blocks_for(n_scenes, cvxnlo::SCENE_BLOCK)), dim3(cvxnlo::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("lo_init_kernel launch");
}

extern "C" int cvxpnpl_ransac_lo_assemble(int64_t n_scenes, int64_t n_active, const int32_t *d_active, const int64_t *d_offsets, int64_t n_total,
                                          const double *d_scene_2d, const double *d_scene_3d, const double *d_R, const double *d_t, const double *d_K,
                                          int32_t K_per_scene, double thresh_k, double *d_B27, double *d_Q45, int32_t *d_count, void *stream)
{
    const char *who = "cvxpnpl_ransac_lo_assemble";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (n_scenes == 0 || n_active == 0) return 0;
    if (int rc = null_among(who, {{"d_R", d_R}, {"d_t", d_t}, {"d_K", d_K}, {"d_B27", d_B27}, {"d_Q45", d_Q45}, {"d_count", d_count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh_k)) return bad_args(who, m);
    cvxnlo::LoAssembleArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.active = d_active; a.off = d_offsets; a.s2 = d_scene_2d; a.s3 = d_scene_3d;
    a.R = d_R; a.t = d_t; a.K = d_K; a.K_per_scene = K_per_scene; a.thresh_k = thresh_k; a.B27 = d_B27; a.Q45 = d_Q45; a.count = d_count;
    hipLaunchKernelGGL(cvxnlo::lo_assemble_active_kernel, dim3((unsigned)n_active), dim3(cvxnlo::LANES), 0, (hipStream_t)stream, a);
    return launched("lo_assemble_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_lo_update(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t cap, double confidence,
                                        const int64_t *d_offsets, int64_t n_total, const double *d_fit_R, const double *d_fit_t,
                                        const int32_t *d_fit_status, const int32_t *d_fit_count, const double *d_K, int32_t K_per_scene,
                                        const double *d_scene_2d, const double *d_scene_3d, double thresh, double *d_io_R, double *d_io_t,
                                        int32_t *d_head, int32_t *d_best, uint8_t *d_mask, const int32_t *d_hyp_used, int32_t *d_lo_taken,
                                        int32_t *d_done, void *stream)
{
    const char *who = "cvxpnpl_ransac_lo_update";
    if (const char *m = check_round(n_scenes, n_active, d_active, d_offsets, n_total, d_scene_2d, d_scene_3d)) return bad_args(who, m);
    if (cap < 0) return bad_args(who, "negative cap");
    if (cvxna::bad_confidence(confidence)) return bad_args(who, "confidence is not inside (0, 1)");
    if (n_scenes == 0 || n_active == 0) return 0;
    if (int rc = null_among(who, {{"d_fit_R", d_fit_R}, {"d_fit_t", d_fit_t}, {"d_fit_status", d_fit_status}, {"d_fit_count", d_fit_count}, {"d_K", d_K},
                                  {"d_io_R", d_io_R}, {"d_io_t", d_io_t}, {"d_head", d_head}, {"d_best", d_best}, {"d_hyp_used", d_hyp_used},
                                  {"d_lo_taken", d_lo_taken}, {"d_done", d_done}}))
        return rc;
    if (n_total > 0 && !d_mask) return bad_args(who, "d_mask is null");
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh)) return bad_args(who, m);
    cvxnlo::LoUpdateArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.cap = cap; a.confidence = confidence; a.active = d_active; a.off = d_offsets;
    a.fit_R = d_fit_R; a.fit_t = d_fit_t; a.fit_status = d_fit_status; a.fit_cnt = d_fit_count; a.K = d_K; a.K_per_scene = K_per_scene;
    a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.thresh = thresh; a.io_R = d_io_R; a.io_t = d_io_t; a.head = d_head; a.best = d_best; a.mask = d_mask;
    a.hyp_used = d_hyp_used; a.lo_taken = d_lo_taken; a.done = d_done;
    hipLaunchKernelGGL(cvxnlo::lo_update_active_kernel, dim3((unsigned)n_active), dim3(cvxnlo::SCENE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("lo_update_active_kernel launch");
}

extern "C" int cvxpnpl_ransac_lo_assemble_host(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *offsets, int64_t n_total,
                                               const double *scene_2d, const double *scene_3d, const double *R, const double *t, const double *K,
                                               int32_t K_per_scene, double thresh_k, double *B27, double *Q45, int32_t *count, int32_t n_threads)
{
    const char *who = "cvxpnpl_ransac_lo_assemble_host";
    if (const char *m = check_sizes(true, n_scenes, n_active, n_total)) return bad_args(who, m);
    if (n_scenes == 0 || n_active == 0) return 0;
    if (!active) return bad_args(who, "active is null");
    if (!offsets) return bad_args(who, "offsets is null");
    if (n_total > 0 && (!scene_2d || !scene_3d)) return bad_args(who, "scene_2d or scene_3d is null");
    if (int rc = null_among(who, {{"R", R}, {"t", t}, {"K", K}, {"B27", B27}, {"Q45", Q45}, {"count", count}})) return rc;
    if (const char *m = check_K_per_scene(K_per_scene)) return bad_args(who, m);
    if (const char *m = check_thresh(thresh_k)) return bad_args(who, m);
    const double th2 = thresh_k * thresh_k;
    cvxh::for_chunks(n_active, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t ai = lo; ai < hi; ++ai) { // the kernel's workgroup
            const int64_t f = active[ai];
            if (f < 0 || f >= n_scenes) continue; // skipped, not clamped
            host_entry(ai, f, offsets, n_total, scene_2d, scene_3d, R, t, K, K_per_scene, th2, B27, Q45, count);
        }
    });
    return 0;
}
