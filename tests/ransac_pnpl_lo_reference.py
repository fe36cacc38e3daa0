"""Reference of local optimisation in adaptive RANSAC over points AND lines, numpy only: it shares no code with
the library.

taken (ransac_lo_reference): the point predicate, with the least relative distance of an r^2 to tau^2.
line_taken: the line predicate of one pose over one scene's lines, with the least relative distance of an end point's |d| to tau:

    l = (a, 1) x (b, 1) / hypot(l_0, l_1)   the image line through the two 2D samples a, b, normalised ONCE per line
    X_c = R P_k + t,  (u, v, w) = K X_c,  d_k = l . (u / w, v / w, 1)          for both 3D end points P_0, P_1
    taken: X_c.z > 0 and |d_k| < tau for both end points  (a NaN compares false: a degenerate 2D line, a = b, is never taken)

first_records / centre: the rule of the centre of the Gram sums -- the first three taken 3D records in the order "points, then lines", a
line giving its two end points; per coordinate their median, fewer than three: the first.
simulate_lo (ransac_lo_reference): the replay of the rounds on GIVEN counts; a point-and-line scene enters with M_f = P_f + L_f.
PnplSceneReplay: the CPU experiment -- the device sampler's draws over the UNION of a scene's correspondences
(synth.philox_minimal_sets(cap, P + L, 4, seed): index c < P is point c, otherwise line c - P), the host build of the device algorithm
(tests/hostsim) for the minimal assembly and solves and for the refits (hostsim.assemble + hostsim.solve_cost_batch on the gathered
points and lines), this module for everything else."""
import numpy as np

from ransac_adaptive_reference import needed
from ransac_lo_reference import pack45, simulate_lo, take_fit, taken, widen  # noqa: F401  (simulate_lo: re-exported for the tests)


def line_taken(l2, l3, K, R, t, thresh, dtype=np.float64):
    """l2 [L,2,2], l3 [L,2,3], K [3,3], R [3,3], t [3] -> (mask [L] bool, margin: min ||d| - tau| / tau over the finite d, inf if none)."""
    l2 = np.asarray(l2, dtype=dtype).reshape(-1, 2, 2)
    l3 = np.asarray(l3, dtype=dtype).reshape(-1, 2, 3)
    K, R, t = (np.asarray(a, dtype=dtype) for a in (K, R, t))
    tau = dtype(thresh)
    if len(l2) == 0:
        return np.zeros(0, dtype=bool), np.inf
    with np.errstate(all="ignore"):
        a, b = l2[:, 0], l2[:, 1]
        l = np.stack([a[:, 1] - b[:, 1], b[:, 0] - a[:, 0], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        l = l * (1.0 / np.hypot(l[:, 0], l[:, 1]))[:, None]
        Xc = l3 @ R.T + t                                   # [L,2,3]
        uvw = Xc @ K.T
        d = l[:, None, 0] * (uvw[..., 0] / uvw[..., 2]) + l[:, None, 1] * (uvw[..., 1] / uvw[..., 2]) + l[:, None, 2]
        near = (Xc[..., 2] > 0) & (np.abs(d) < tau)         # [L,2]
        mask = near[:, 0] & near[:, 1]
        fin = np.isfinite(d)
        margin = float(np.min(np.abs(np.abs(d[fin]) - tau) / tau)) if fin.any() and tau > 0 else np.inf
    return mask, margin


def scene_taken(pts_2d, pts_3d, line_2d, line_3d, K, R, t, thresh):
    """(mask_pts [P], mask_lines [L], least margin) of one pose over one scene"""
    if len(pts_3d):
        mp, m1 = taken(pts_2d, pts_3d, K, R, t, thresh)
    else:
        mp, m1 = np.zeros(0, dtype=bool), np.inf
    ml, m2 = line_taken(line_2d, line_3d, K, R, t, thresh)
    return mp, ml, min(m1, m2)


def first_records(pts_3d, line_3d, mask_pts, mask_lines):
    """the first three taken 3D records [<= 3, 3]: up to three points in scene order, then -- while fewer than three records -- the end
    points of up to two lines in scene order"""
    rec = [np.asarray(pts_3d, dtype=np.float64).reshape(-1, 3)[m] for m in np.flatnonzero(mask_pts)[:3]]
    for m in np.flatnonzero(mask_lines):
        if len(rec) >= 3:
            break
        rec.extend(np.asarray(line_3d, dtype=np.float64).reshape(-1, 2, 3)[m])
    return np.array(rec[:3]).reshape(-1, 3)


def centre(pts_3d, line_3d, mask_pts, mask_lines):
    """per coordinate the median of the first three taken records; fewer than three: the first; none: the origin"""
    rec = first_records(pts_3d, line_3d, mask_pts, mask_lines)
    if len(rec) == 0:
        return np.zeros(3)
    return np.median(rec, axis=0) if len(rec) == 3 else rec[0].copy()


def count_poses(scene, R, t, status, thresh):
    """inlier counts (points plus lines, a line once) of the poses (R, t)[h] over one scene; a status outside (0, 2) counts 0"""
    c = np.zeros(len(R), dtype=np.int64)
    for h in range(len(R)):
        mp, ml, _ = scene_taken(scene["pts_2d"], scene["pts_3d"], scene["line_2d"], scene["line_3d"], scene["K"], R[h], t[h], thresh)
        c[h] = int(mp.sum()) + int(ml.sum())
    return np.where(np.isin(status, (0, 2)), c, 0)


class PnplSceneReplay:
    """One scene of the experiment (a dict of synth.make_ransac_pnpl): its draws are the device sampler's over the union, its minimal
    costs and solves the host build's, solved round by round on demand and kept, so that the plain call and the LO call share them."""

    def __init__(self, scene, seed, cap, thresh, eps=1e-6, max_iters=100):
        import hostsim
        from cvxpnpl_amd import synth

        self.hs, self.sc = hostsim, scene
        self.P, self.L = len(scene["pts_3d"]), len(scene["line_3d"])
        self.M, self.cap, self.thresh = self.P + self.L, cap, thresh
        self.idx = synth.philox_minimal_sets(cap, self.M, 4, seed)
        self.opts = dict(eps=eps, max_iters=max_iters)
        self.rounds = {}

    def _gathered_cost(self, mask_pts, mask_lines):
        s = self.sc
        return self.hs.assemble(s["pts_2d"][mask_pts] if self.P else None, s["pts_3d"][mask_pts] if self.P else None,
                                s["line_2d"][mask_lines] if self.L else None, s["line_3d"][mask_lines] if self.L else None, s["K"])

    def round(self, h0, Hr):
        """(R, t, count) of hypotheses h0 .. h0 + Hr - 1: each set assembled as the sampler does (its points in draw order, then its
        lines in draw order) and solved at the cost seam with the minimal solves' option (rescue_from = 32)"""
        if (h0, Hr) not in self.rounds:
            Q45, B27 = np.zeros((Hr, 45)), np.zeros((Hr, 27))
            for j, pick in enumerate(self.idx[h0:h0 + Hr]):
                ip, il = [c for c in pick if c < self.P], [c - self.P for c in pick if c >= self.P]
                rc, B, Q = self._gathered_cost(np.array(ip, dtype=np.int64), np.array(il, dtype=np.int64))
                Q45[j], B27[j] = (pack45(Q), B.reshape(27)) if rc == 0 else (np.nan, np.nan)
            sol = self.hs.solve_cost_batch(Q45, B27, self.hs.default_opts(rescue_from=32, **self.opts))
            self.rounds[(h0, Hr)] = (sol["R"], sol["t"], count_poses(self.sc, sol["R"], sol["t"], sol["status"], self.thresh))
        return self.rounds[(h0, Hr)]

    def count(self, R, t, thresh):
        mp, ml, _ = scene_taken(self.sc["pts_2d"], self.sc["pts_3d"], self.sc["line_2d"], self.sc["line_3d"], self.sc["K"], R, t, thresh)
        return mp, ml, int(mp.sum()) + int(ml.sum())

    def refit(self, R, t, thresh_k):
        """the LO solve of one step at the pose (R, t): (R, t, status, size of the set) -- status 3 when fewer than three are taken or
        the assembly is singular; solved with the call's own options, not the minimal solves'"""
        mp, ml, cnt = self.count(R, t, thresh_k)
        if cnt < 3:
            return R, t, 3, cnt
        rc, B, Q = self._gathered_cost(mp, ml)
        if rc != 0:
            return R, t, 3, cnt
        fit = self.hs.solve_cost_batch(pack45(Q)[None], B.reshape(1, 27), self.hs.default_opts(**self.opts))
        return fit["R"][0], fit["t"][0], int(fit["status"][0]), cnt

    def run(self, p, round_hyp, local_opt=0, lo_widen=1.0):
        """the rounds of the scene: {"hyp_used", "best", "lo_taken", "rounds"}"""
        best, pose, lo_taken, h0, rounds = -1, None, 0, 0, 0
        while h0 < self.cap:
            Hr = min(round_hyp, self.cap - h0)
            R, t, c = self.round(h0, Hr)
            j = int(np.argmax(c))
            if c[j] > best:
                best, pose = int(c[j]), (R[j], t[j])
            drawn = h0 + Hr
            done = drawn >= self.cap or drawn >= needed(best, self.M, p)
            for k in range(local_opt):
                fR, ft, st, cnt = self.refit(pose[0], pose[1], self.thresh * widen(k, local_opt, lo_widen))
                n_new = self.count(fR, ft, self.thresh)[2]
                if take_fit(st, cnt, n_new, best):
                    best, pose, lo_taken = n_new, (fR, ft), lo_taken + 1
                done = done or drawn >= needed(best, self.M, p)
            h0, rounds = drawn, rounds + 1
            if done:
                break
        return {"hyp_used": h0, "best": best, "lo_taken": lo_taken, "rounds": rounds}
