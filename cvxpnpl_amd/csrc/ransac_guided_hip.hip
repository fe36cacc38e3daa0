// ransac_guided_hip.hip -- entry points of guided RANSAC over many scenes (include/cvxpnpl_amd_ransac_guided.h), built as
// libcvxpnpl_amd_ransac_guided.so.  The kernels are ransac_guided_kernel.h, the pool rule and the ranking order ransac_guided_core.h, the
// shared checks and the slab launch ransac_entry.h.  Every entry point checks its arguments before it launches anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cvxpnpl_amd_ransac_guided.h"
#include "host_pool.h"
#include "ransac_entry.h"
#include "ransac_guided_kernel.h"

using namespace cvxne;

namespace {

// what the two samplers share: the sizes, each under its own name and checked before a zero-size call returns ...
const char *check_guided_sizes(int64_t n_scenes, int64_t n_total, int32_t pool_full)
{
    if (n_scenes < 0) return "negative n_scenes";
    if (n_total < 0) return "negative n_total";
    if (n_scenes > 0x7fffffffLL) return "more scenes than an int32 index holds";
    if (pool_full < 0) return "negative pool_full";
    return nullptr;
}

// ... and the pointers of a call that launches: the scene set, the ranking, the outputs.  Returns a message or null.
const char *check_draw(const int64_t *off, int64_t n_total, const double *s2, const double *s3, int32_t pool_full, const uint64_t *seeds,
                       const int32_t *order, const double *K, const double *p2, const double *p3, const double *Kh)
{
    if (const char *m = check_scene_ptrs(off, n_total, s2, s3, "d_scene_2d or d_scene_3d is null")) return m;
    if (!seeds) return "d_seeds is null";
    if (pool_full > 0 && !order) return "d_order is null";
    if (!p2 || !p3) return "d_pts_2d or d_pts_3d is null";
    if ((K == nullptr) != (Kh == nullptr)) return "d_K and d_K_hyp go together";
    return nullptr;
}

} // namespace

extern "C" const char *cvxpnpl_ransac_guided_last_error(void) { return err_buf(); }

extern "C" int32_t cvxpnpl_ransac_guided_pool_host(int32_t h, int32_t n_corr, int32_t pool_full)
{
    if (h < 0 || n_corr < cvxng::MINIMAL || pool_full < 0) return -1;
    return cvxng::pool_size(h, n_corr, pool_full);
}

extern "C" int cvxpnpl_ransac_guided_rank_host(int64_t n_scenes, const int64_t *offsets, int64_t n_total, const double *quality, int32_t *order,
                                               int32_t n_threads)
{
    const char *who = "cvxpnpl_ransac_guided_rank_host";
    if (n_scenes < 0) return bad_args(who, "negative n_scenes");
    if (n_total < 0) return bad_args(who, "negative n_total");
    if (n_scenes == 0 || n_total == 0) return 0;
    if (!offsets) return bad_args(who, "offsets is null");
    if (!quality) return bad_args(who, "quality is null");
    if (!order) return bad_args(who, "order is null");
    cvxh::for_chunks(n_scenes, n_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t f = lo; f < hi; ++f) {
            const cvxn::Slice sl = cvxn::scene_slice(offsets, f, n_total);
            const int64_t beg = sl.beg, n = sl.n;
            const double *q = quality + beg;
            for (int64_t m = 0; m < n; ++m) { // the kernel's lane m
                const double key = cvxng::quality_key(q[m]);
                int64_t rank = 0;
                for (int64_t j = 0; j < n; ++j) rank += cvxng::ranks_before(cvxng::quality_key(q[j]), (int32_t)j, key, (int32_t)m) ? 1 : 0;
                order[beg + rank] = (int32_t)m;
            }
        }
    });
    return 0;
}

extern "C" int cvxpnpl_ransac_guided_rank(int64_t n_scenes, const int64_t *d_offsets, int64_t n_total, int32_t max_corr, const double *d_quality,
                                          int32_t *d_order, void *stream)
{
    const char *who = "cvxpnpl_ransac_guided_rank";
    if (n_scenes < 0) return bad_args(who, "negative n_scenes");
    if (n_total < 0) return bad_args(who, "negative n_total");
    if (max_corr < 0) return bad_args(who, "negative max_corr");
    if (n_scenes > 0x7fffffffLL) return bad_args(who, "more scenes than an int32 index holds");
    if (n_scenes == 0 || n_total == 0 || max_corr == 0) return 0;
    if (!d_offsets) return bad_args(who, "d_offsets is null");
    if (!d_quality) return bad_args(who, "d_quality is null");
    if (!d_order) return bad_args(who, "d_order is null");
    cvxng::RankArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.off = d_offsets; a.quality = d_quality; a.order = d_order;
    launch_slabs(cvxng::rank_quality_kernel, max_corr, cvxng::SCENE_BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("rank_quality_kernel launch");
}

extern "C" int cvxpnpl_ransac_guided_sample(int64_t n_scenes, int32_t n_hyp, int32_t pool_full, const int64_t *d_offsets, int64_t n_total,
                                            const uint64_t *d_seeds, const int32_t *d_order, const double *d_scene_2d, const double *d_scene_3d,
                                            const double *d_K, int32_t *d_idx, double *d_pts_2d, double *d_pts_3d, double *d_K_hyp, void *stream)
{
    const char *who = "cvxpnpl_ransac_guided_sample";
    if (const char *m = check_guided_sizes(n_scenes, n_total, pool_full)) return bad_args(who, m);
    if (n_hyp < 0) return bad_args(who, "negative n_hyp");
    if (n_scenes == 0 || n_hyp == 0) return 0;
    if (const char *m = check_draw(d_offsets, n_total, d_scene_2d, d_scene_3d, pool_full, d_seeds, d_order, d_K, d_pts_2d, d_pts_3d, d_K_hyp))
        return bad_args(who, m);
    cvxng::SampleGuidedArgs a;
    a.n_scenes = n_scenes; a.n_total = n_total; a.n_hyp = n_hyp; a.pool_full = pool_full; a.off = d_offsets; a.seed = d_seeds; a.order = d_order;
    a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.K = d_K; a.idx = d_idx; a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.Kh = d_K_hyp;
    launch_slabs(cvxng::sample_guided_kernel, n_hyp, cvxng::SCENE_BLOCK, n_scenes, a, &decltype(a)::scene0, stream);
    return launched("sample_guided_kernel launch");
}

extern "C" int cvxpnpl_ransac_guided_sample_active(int64_t n_scenes, int64_t n_active, const int32_t *d_active, int32_t hyp0, int32_t n_round,
                                                   int32_t cap, int32_t pool_full, const int64_t *d_offsets, int64_t n_total,
                                                   const uint64_t *d_seeds, const int32_t *d_order, const double *d_scene_2d,
                                                   const double *d_scene_3d, const double *d_K, int32_t *d_idx, double *d_pts_2d,
                                                   double *d_pts_3d, double *d_K_hyp, void *stream)
{
    const char *who = "cvxpnpl_ransac_guided_sample_active";
    if (n_active < 0) return bad_args(who, "negative n_active");
    if (n_active > 0x7fffffffLL) return bad_args(who, "more active scenes than an int32 index holds");
    if (const char *m = check_guided_sizes(n_scenes, n_total, pool_full)) return bad_args(who, m);
    if (hyp0 < 0) return bad_args(who, "negative hyp0");
    if (n_round < 0) return bad_args(who, "negative n_round");
    if (cap < 0) return bad_args(who, "negative cap");
    if ((int64_t)hyp0 + n_round > (int64_t)cap) return bad_args(who, "hyp0 + n_round exceeds cap");
    if (n_scenes == 0 || n_active == 0 || n_round == 0) return 0;
    if (!d_active) return bad_args(who, "d_active is null");
    if (const char *m = check_draw(d_offsets, n_total, d_scene_2d, d_scene_3d, pool_full, d_seeds, d_order, d_K, d_pts_2d, d_pts_3d, d_K_hyp))
        return bad_args(who, m);
    cvxng::SampleGuidedActiveArgs a;
    a.n_active = n_active; a.n_scenes = n_scenes; a.n_total = n_total; a.hyp0 = hyp0; a.n_round = n_round; a.pool_full = pool_full;
    a.active = d_active; a.off = d_offsets; a.seed = d_seeds; a.order = d_order; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.K = d_K; a.idx = d_idx;
    a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.Kh = d_K_hyp;
    launch_slabs(cvxng::sample_guided_active_kernel, n_round, cvxng::SCENE_BLOCK, n_active, a, &decltype(a)::act0, stream);
    return launched("sample_guided_active_kernel launch");
}
