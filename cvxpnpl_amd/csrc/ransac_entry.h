// ransac_entry.h -- what the entry points of the nine RANSAC libraries (ransac, ransac_pnpl, ransac_adaptive, ransac_guided,
// ransac_pnpl_adaptive, ransac_msac, ransac_lo, ransac_pnpl_lo) share around their kernels: the error text, the argument contract of a
// scenes call and of a round, the pointers of a call by name, and the launch of a kernel whose grid is (hypotheses, scenes or active
// entries).  Host-only.  Every function is inline and hidden: each library keeps
// a copy of its own -- its own thread-local message -- and exports nothing of this.
//
// The checks return a message or null; an entry point runs them in this order: the sizes and -- a call that launches -- the pointers of
// the scene set (check_scenes / check_round), its own sizes, the zero-size no-op, its own pointers, K_per_scene, thresh.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "entry_error.h"

#define CVXNE_FN inline __attribute__((visibility("hidden")))

namespace cvxne {

// the error text: entry_error.h
using cvxee::bad_args;
using cvxee::err_buf;
using cvxee::launched;

// ---- the argument contract ----

// The sizes of a scenes call (n_active = 0) or of a round.  int32_limit: the kernels index scenes and active entries by an int32; the
// adaptive, guided and pnpl-adaptive libraries refuse a count beyond it here, the first two libraries only where one launch holds every
// scene (check_one_launch).
CVXNE_FN const char *check_sizes(bool int32_limit, int64_t n_scenes, int64_t n_active, int64_t n_pts, int64_t n_lines = 0)
{
    if (n_scenes < 0 || n_active < 0 || n_pts < 0 || n_lines < 0) return "negative size";
    if (int32_limit && (n_scenes > 0x7fffffffLL || n_active > 0x7fffffffLL)) return "more scenes than an int32 index holds";
    return nullptr;
}

CVXNE_FN const char *check_one_launch(int64_t n_scenes) { return n_scenes > 0x7fffffffLL ? "more scenes than one launch holds" : nullptr; }

// the pointers of a scene set, point form and point-and-line form
// (the guided library names the two scene pointers in its message: no_scene)
CVXNE_FN const char *check_scene_ptrs(const int64_t *off, int64_t n_total, const double *s2, const double *s3,
                                      const char *no_scene = "a scene pointer is null")
{
    if (!off) return "d_offsets is null";
    if (n_total > 0 && (!s2 || !s3)) return no_scene;
    return nullptr;
}

CVXNE_FN const char *check_pnpl_ptrs(const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines, const double *p2, const double *p3,
                                     const double *l2, const double *l3)
{
    if (!off_p || !off_l) return "d_pt_offsets or d_ln_offsets is null";
    if (n_pts > 0 && (!p2 || !p3)) return "a point pointer is null";
    if (n_lines > 0 && (!l2 || !l3)) return "a line pointer is null";
    return nullptr;
}

// What every entry point of a scenes call shares: the sizes, then -- scenes given -- the offsets and the packed scene.
CVXNE_FN const char *check_scenes(bool int32_limit, int64_t n_scenes, const int64_t *off, int64_t n_total, const double *s2, const double *s3)
{
    if (const char *m = check_sizes(int32_limit, n_scenes, 0, n_total)) return m;
    return n_scenes > 0 ? check_scene_ptrs(off, n_total, s2, s3) : nullptr;
}

// ... and of a round: the active list before the scene set
CVXNE_FN const char *check_round(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *off, int64_t n_total, const double *s2,
                                 const double *s3)
{
    if (const char *m = check_sizes(true, n_scenes, n_active, n_total)) return m;
    if (n_scenes == 0 || n_active == 0) return nullptr;
    return !active ? "d_active is null" : check_scene_ptrs(off, n_total, s2, s3);
}

// The same for points and lines; both fill the scene set s (cvxnl::SceneSet), K left to the entry point.
template <class S>
CVXNE_FN void fill_scene_set(S &s, int64_t n_scenes, const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines, const double *p2,
                             const double *p3, const double *l2, const double *l3)
{
    s.n_scenes = n_scenes; s.n_pts = n_pts; s.n_lines = n_lines; s.off_p = off_p; s.off_l = off_l; s.p2 = p2; s.p3 = p3; s.l2 = l2; s.l3 = l3;
    s.K = nullptr; s.K_per_scene = 0;
}

template <class S>
CVXNE_FN const char *check_pnpl_scenes(bool int32_limit, int64_t n_scenes, const int64_t *off_p, int64_t n_pts, const int64_t *off_l, int64_t n_lines,
                                       const double *p2, const double *p3, const double *l2, const double *l3, S &s)
{
    if (const char *m = check_sizes(int32_limit, n_scenes, 0, n_pts, n_lines)) return m;
    if (n_scenes > 0)
        if (const char *m = check_pnpl_ptrs(off_p, n_pts, off_l, n_lines, p2, p3, l2, l3)) return m;
    fill_scene_set(s, n_scenes, off_p, n_pts, off_l, n_lines, p2, p3, l2, l3);
    return nullptr;
}

template <class S>
CVXNE_FN const char *check_pnpl_round(int64_t n_scenes, int64_t n_active, const int32_t *active, const int64_t *off_p, int64_t n_pts,
                                      const int64_t *off_l, int64_t n_lines, const double *p2, const double *p3, const double *l2, const double *l3,
                                      S &s)
{
    if (const char *m = check_sizes(true, n_scenes, n_active, n_pts, n_lines)) return m;
    if (n_scenes > 0 && n_active > 0) {
        if (!active) return "d_active is null";
        if (const char *m = check_pnpl_ptrs(off_p, n_pts, off_l, n_lines, p2, p3, l2, l3)) return m;
    }
    fill_scene_set(s, n_scenes, off_p, n_pts, off_l, n_lines, p2, p3, l2, l3);
    return nullptr;
}

// the pointers of a call that launches, each under its own name: the first null one becomes the message
struct Named { const char *name; const void *p; };
template <int N>
CVXNE_FN int null_among(const char *who, const Named (&ptrs)[N])
{
    for (const Named &n : ptrs)
        if (!n.p) return cvxee::fail(-1, "%s: bad arguments (%s is null)", who, n.name);
    return 0;
}

// the budget of a round: hypotheses hyp0 .. hyp0 + n_round - 1 of at most cap
CVXNE_FN const char *check_budget(int32_t hyp0, int32_t n_round, int32_t cap)
{
    if (hyp0 < 0 || n_round < 0 || cap < 0) return "negative hyp0, n_round or cap";
    if ((int64_t)hyp0 + n_round > (int64_t)cap) return "hyp0 + n_round exceeds cap";
    return nullptr;
}

CVXNE_FN const char *check_K_per_scene(int32_t K_per_scene) { return K_per_scene != 0 && K_per_scene != 1 ? "K_per_scene is 0 or 1" : nullptr; }

CVXNE_FN bool bad_thresh(double thresh) { return !(thresh >= 0.0) || thresh > 1.7e308; }

CVXNE_FN const char *check_thresh(double thresh) { return bad_thresh(thresh) ? "thresh is not a finite non-negative number" : nullptr; }

// ---- the launches ----

constexpr int64_t GRID_Y = 65535; // scenes (or active entries) per launch of a kernel whose grid is (x, scenes)

CVXNE_FN unsigned blocks_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// A kernel whose grid is (nx threads in blocks of `block`, n scenes or active entries), launched in slabs of GRID_Y; a.*start receives the
// first scene (or entry) of each slab.
template <class A>
CVXNE_FN void launch_slabs(void (*kernel)(A), int64_t nx, int block, int64_t n, A &a, int64_t A::*start, void *stream)
{
    const unsigned gx = blocks_for(nx, block);
    for (int64_t y0 = 0; y0 < n; y0 += GRID_Y) {
        a.*start = y0;
        const int64_t ny = n - y0 < GRID_Y ? n - y0 : GRID_Y;
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)ny), dim3(block), 0, (hipStream_t)stream, a);
    }
}

} // namespace cvxne
