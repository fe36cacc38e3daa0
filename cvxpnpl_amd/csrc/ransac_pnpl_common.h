// ransac_pnpl_common.h -- what the two libraries of RANSAC over points AND lines share (libcvxpnpl_amd_ransac_pnpl.so:
// ransac_pnpl_kernel.h, every scene the same budget; libcvxpnpl_amd_ransac_pnpl_adaptive.so: ransac_pnpl_adaptive_kernel.h, rounds over the
// active scenes and guided draws): the scene set of two packed arrays, the line inlier predicate, a hypothesis from its draw to its
// cost, the scoring of one scene through LDS and the masks of one pose by a workgroup.  ONE definition of each, and no kernel, as ransac_common.h: a
// library that includes this header compiles nothing it does not launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "problem_io.h"
#include "ransac_common.h"
#include "solver_core.h"

namespace cvxnl {

using cvxn::Camera;
using cvxn::Slice;

using cvxn::POINT_TILE;
using cvxn::SCENE_WAVES;
constexpr int BLOCK = cvxn::SCENE_BLOCK; // (the name the entry files launch with)
constexpr int LINE_TILE = 256;           // lines per LDS tile: 9 doubles each (18 KB), in the buffer of POINT_TILE points
constexpr int TILE_DOUBLES = POINT_TILE * 5;
static_assert(LINE_TILE * 9 <= TILE_DOUBLES && LINE_TILE <= BLOCK, "a line tile fits the buffer and is staged one line per lane");

// the scene set every kernel sees
struct SceneSet {
    int64_t n_scenes, n_pts, n_lines;
    const int64_t *off_p, *off_l;  // [n_scenes + 1] each
    const double *p2, *p3;         // [n_pts][2], [n_pts][3]
    const double *l2, *l3;         // [n_lines][4] (u0 v0 u1 v1), [n_lines][6] (P0 P1)
    const double *K;               // [9] or [n_scenes][9]
    int32_t K_per_scene;
};
struct Scene {
    int32_t P, L;                  // L is cut so that P + L fits an int32
    const double *p2, *p3, *l2, *l3;
    int64_t beg_p, beg_l;
    const double *K;
};
__device__ inline Scene scene_of(const SceneSet &s, int64_t f)
{
    const Slice sp = cvxn::scene_slice(s.off_p, f, s.n_pts), sl = cvxn::scene_slice(s.off_l, f, s.n_lines);
    Scene sc;
    sc.P = sp.n;
    sc.L = sl.n > 0x7fffffff - sp.n ? 0x7fffffff - sp.n : sl.n;
    sc.beg_p = sp.beg; sc.beg_l = sl.beg;
    sc.p2 = s.p2 + sp.beg * 2; sc.p3 = s.p3 + sp.beg * 3; // (never followed where P or L is 0)
    sc.l2 = s.l2 + sl.beg * 4; sc.l3 = s.l3 + sl.beg * 6;
    sc.K = s.K + (s.K_per_scene ? f * 9 : 0);
    return sc;
}

// ---- the line inlier predicate, beside cvxn::is_inlier for points: ONE statement of it, used by the scoring kernels (counts) and by the
// workgroup kernels (masks).  A 2D line is two pixel samples a, b on it; the image line is l = (a, 1) x (b, 1), and l . (u, v, 1) /
// hypot(l_0, l_1) is the signed distance of pixel (u, v) from it.  A line is an inlier of a pose when BOTH 3D end points have depth > 0
// and BOTH projected end points lie within thresh pixels of the image line.  image_line normalises l once (the scoring kernels do it
// once per tile); a degenerate line (a = b) has hypot = 0 and gets l_0 = 0 * inf = NaN, so it compares false under every pose, as a NaN
// pose does on every line.
__device__ inline void image_line(double ax, double ay, double bx, double by, double *l)
{
    const double l0 = ay - by, l1 = bx - ax, l2 = ax * by - ay * bx;
    const double inv = 1.0 / hypot(l0, l1);
    l[0] = l0 * inv; l[1] = l1 * inv; l[2] = l2 * inv;
}
__device__ inline bool end_point_near(const Camera &c, const double *l, double X, double Y, double Z, double thresh)
{
    const double u = c.M[0] * X + c.M[1] * Y + c.M[2] * Z + c.M[3];
    const double v = c.M[4] * X + c.M[5] * Y + c.M[6] * Z + c.M[7];
    const double w = c.M[8] * X + c.M[9] * Y + c.M[10] * Z + c.M[11];
    const double depth = c.r2[0] * X + c.r2[1] * Y + c.r2[2] * Z + c.t2;
    const double d = l[0] * (u / w) + l[1] * (v / w) + l[2];
    return depth > 0.0 && (fabs(d) < thresh);
}
__device__ inline bool is_line_inlier_normalised(const Camera &c, const double *l /* image_line */, const double *e /* P0 P1 */, double thresh)
{
    return end_point_near(c, l, e[0], e[1], e[2], thresh) && end_point_near(c, l, e[3], e[4], e[5], thresh);
}
__device__ inline bool is_line_inlier(const Camera &c, const double *ab /* u0 v0 u1 v1 */, const double *e /* P0 P1 */, double thresh)
{
    double l[3];
    image_line(ab[0], ab[1], ab[2], ab[3], l);
    return is_line_inlier_normalised(c, l, e, thresh);
}

// ---- one hypothesis, from the draw to the cost, by one lane: hypothesis h (index within the scene: the Philox counter) of scene sc,
// written as problem g.  The draw is that of cvxn::uniform_hypothesis (cvxn::draw_minimal_set: same key, same counter) over the first
// `pool` of the scene's M_f = P_f + L_f correspondences; index c < P_f is point c, otherwise line c - P_f.  ranked (optional): the
// scene's ranking, the draw is then a set of ranks and the set is ranked[pick[j]]; an entry outside [0, M_f) never becomes an address,
// the hypothesis is then written as that of a scene too short to draw from.  The lane assembles its set in place, in the order and about
// the centre cvxa / cvx::assemble use on the gathered set: points in draw order, then lines in draw order; centre = cvx::shift_centre of
// the first three 3D records in that order (a set of four correspondences always has at least four records).  Fewer than four
// correspondences, a singular K or no set: NaN cost and idx = -1.
__device__ inline void minimal_hypothesis(const Scene &sc, uint64_t seed, int32_t h, int32_t pool /* 4 .. M_f */, const int32_t *ranked, int64_t g,
                                          int32_t *idx /* optional */, double *Q45, double *B27)
{
    const int32_t M = sc.P + sc.L;
    double Kc[9], Ki[9], det;
#pragma unroll
    for (int i = 0; i < 9; ++i) Kc[i] = sc.K[i];
    cvx::inv3(Kc, Ki, det);
    bool drawable = M >= 4 && (det == det) && det != 0.0; // what idx reports: apart from what gram_finish finds in the set itself
    int pick[4] = {-1, -1, -1, -1};
    double c[3] = {0.0, 0.0, 0.0};
    cvx::Gram gm;
    cvx::gram_zero(gm);
    if (M >= 4) {
        cvxn::draw_minimal_set(pool, seed, (uint32_t)h, pick); // 0 .. pool - 1 <= M - 1 by construction
        bool have_set = true;
        if (ranked) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pick[j] = ranked[pick[j]];
                have_set = have_set && pick[j] >= 0 && pick[j] < M;
            }
            drawable = drawable && have_set;
        }
        if (have_set) {
            // the first three 3D records of the set: its points in draw order, then the end points of its lines in draw order
            double first3[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int nrec = 0;
            auto put = [&](const double *r) { // (static indices: registers)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    first3[k] = nrec == 0 ? r[k] : first3[k];
                    first3[3 + k] = nrec == 1 ? r[k] : first3[3 + k];
                    first3[6 + k] = nrec == 2 ? r[k] : first3[6 + k];
                }
                ++nrec;
            };
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pick[j] < sc.P) put(sc.p3 + 3 * (int64_t)pick[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pick[j] >= sc.P && nrec < 3) {
                    const double *e = sc.l3 + 6 * (int64_t)(pick[j] - sc.P);
                    put(e);
                    put(e + 3);
                }
            cvx::shift_centre(3, first3, 0, nullptr, c);
#pragma unroll 1
            for (int j = 0; j < 4; ++j) { // (rolled: one copy of the 60 accumulations per kind)
                const int q = j == 0 ? pick[0] : (j == 1 ? pick[1] : (j == 2 ? pick[2] : pick[3]));
                if (q < sc.P) {
                    const double *x = sc.p2 + 2 * (int64_t)q, *X = sc.p3 + 3 * (int64_t)q;
                    cvx::gram_add_point(gm, Ki, x[0], x[1], X[0] - c[0], X[1] - c[1], X[2] - c[2]);
                }
            }
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int q = j == 0 ? pick[0] : (j == 1 ? pick[1] : (j == 2 ? pick[2] : pick[3]));
                if (q >= sc.P) {
                    const double *x = sc.l2 + 4 * (int64_t)(q - sc.P), *e = sc.l3 + 6 * (int64_t)(q - sc.P);
                    const double ab[4] = {x[0], x[1], x[2], x[3]};
                    const double es[6] = {e[0] - c[0], e[1] - c[1], e[2] - c[2], e[3] - c[0], e[4] - c[1], e[5] - c[2]};
                    cvx::gram_add_line(gm, Ki, ab, es);
                }
            }
        }
    }
    double B[27], Q9[45];
    const bool ok = cvx::gram_finish(gm, B, Q9) && drawable;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j]; // t = -B' r - R c
    if (idx) {
#pragma unroll
        for (int j = 0; j < 4; ++j) idx[g * 4 + j] = drawable ? pick[j] : -1; // fewer than four correspondences, a singular K or no set
    }
#pragma unroll
    for (int i = 0; i < 27; ++i) B27[g * 27 + i] = ok ? B[i] : NAN;
#pragma unroll
    for (int i = 0; i < 45; ++i) Q45[g * 45 + i] = ok ? Q9[i] : NAN;
}

// ---- the inliers of one pose per LANE over one scene, by a workgroup of BLOCK lanes.  The scene's points go through LDS a tile at a
// time and are broadcast to the lanes (cvxn::score_points); then its lines, a tile of end points plus the NORMALISED image
// line, computed once per tile by the lane that stages the line.  Every lane of the workgroup calls it (barriers); a lane that is not
// usable counts nothing.  Returns point inliers + line inliers of the lane's pose.
__device__ inline int score_scene(double *tile /* LDS, TILE_DOUBLES */, const Scene &sc, const Camera &cam, bool usable, double thresh)
{
    int cnt = cvxn::score_points<int64_t>(tile, sc.P, sc.p2, sc.p3, cam, usable, thresh * thresh);
    for (int64_t base = 0; base < sc.L; base += LINE_TILE) {
        const int n = sc.L - base < LINE_TILE ? (int)(sc.L - base) : LINE_TILE;
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const int64_t m = base + (int)threadIdx.x;
            const int i = threadIdx.x;
#pragma unroll
            for (int k = 0; k < 6; ++k) tile[i * 9 + k] = sc.l3[m * 6 + k];
            double l[3];
            image_line(sc.l2[m * 4], sc.l2[m * 4 + 1], sc.l2[m * 4 + 2], sc.l2[m * 4 + 3], l);
            tile[i * 9 + 6] = l[0]; tile[i * 9 + 7] = l[1]; tile[i * 9 + 8] = l[2];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            cnt += usable && is_line_inlier_normalised(cam, tile + i * 9 + 6, tile + i * 9, thresh) ? 1 : 0;
    }
    return cnt;
}

// inliers of ONE pose over one scene's points and lines, by the lanes of one workgroup: writes both masks (optional, together) and returns
// points + lines to every lane
__device__ inline int block_inliers(const Camera &cam, const Scene &sc, double thresh, uint8_t *mask_p, uint8_t *mask_l, int *red /* LDS, SCENE_WAVES ints */)
{
    const double th2 = thresh * thresh;
    int cnt = 0;
    for (int64_t m = threadIdx.x; m < sc.P; m += BLOCK) { // (int64: m + BLOCK may pass 2^31 where P_f is within a stride of it)
        const bool in = cvxn::is_inlier(cam, sc.p3[3 * m], sc.p3[3 * m + 1], sc.p3[3 * m + 2], sc.p2[2 * m], sc.p2[2 * m + 1], th2);
        cnt += in ? 1 : 0;
        if (mask_p) mask_p[m] = in ? 1 : 0;
    }
    for (int64_t m = threadIdx.x; m < sc.L; m += BLOCK) {
        const double *x = sc.l2 + 4 * m, *e = sc.l3 + 6 * m;
        const double ab[4] = {x[0], x[1], x[2], x[3]}, es[6] = {e[0], e[1], e[2], e[3], e[4], e[5]};
        const bool in = is_line_inlier(cam, ab, es, thresh);
        cnt += in ? 1 : 0;
        if (mask_l) mask_l[m] = in ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int wv = 0; wv < SCENE_WAVES; ++wv) tot += red[wv];
    return tot;
}

} // namespace cvxnl
