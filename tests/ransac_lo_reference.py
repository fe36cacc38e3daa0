"""Reference of local optimisation in adaptive RANSAC, numpy only: it shares no code with the library.

taken: the inlier predicate of one pose over one scene, with the least distance of an r^2 to the threshold:

    X_c = R P + t,  (u, v, w) = K X_c,  r^2 = |(u / w, v / w) - x|^2,  taken: X_c.z > 0 and r^2 < tau^2  (a NaN compares false)

widen: the schedule m_k = 1 + (w - 1)(n - 1 - k) / max(n - 1, 1) of the n steps of a round.
take_fit: the acceptance rule of a refit.
simulate_lo: ransac_adaptive_reference.simulate's replay of the rounds with the LO rule applied on GIVEN refit counts.
SceneReplay: the CPU experiment -- the device sampler's draws, the host build of the device algorithm (tests/hostsim) for the minimal
solves and for the refits (hostsim.assemble + hostsim.solve_cost_batch on the gathered inliers), this module for everything else."""
import numpy as np

from ransac_adaptive_reference import needed


def taken(x, X, K, R, t, thresh, dtype=np.float64):
    """x [M,2], X [M,3], K [3,3], R [3,3], t [3] -> (mask [M] bool, margin: min |r^2 - tau^2| / tau^2 over the finite r^2, inf if none)."""
    x, X, K, R, t = (np.asarray(a, dtype=dtype) for a in (x, X, K, R, t))
    th2 = dtype(thresh) * dtype(thresh)
    with np.errstate(all="ignore"):
        Xc = X @ R.T + t
        uvw = Xc @ K.T
        du = uvw[:, 0] / uvw[:, 2] - x[:, 0]
        dv = uvw[:, 1] / uvw[:, 2] - x[:, 1]
        r2 = du * du + dv * dv
        mask = (Xc[:, 2] > 0) & (r2 < th2)
        fin = np.isfinite(r2)
        margin = float(np.min(np.abs(r2[fin] - th2) / th2)) if fin.any() and th2 > 0 else np.inf
    return mask, margin


def widen(k, n, w):
    """m_k of step k of n: w in the first step, 1 in the last, 1 for n = 1."""
    return 1.0 + (float(w) - 1.0) * (n - 1 - k) / max(n - 1, 1)


def take_fit(status, fit_cnt, n_new, best):
    """a refit is taken when it is usable (status 0 or 2, fitted to at least four) and counts at least the running best: it wins a tie"""
    return int(status) in (0, 2) and int(fit_cnt) >= 4 and int(n_new) >= int(best)


def simulate_lo(counts, status, sizes, lo_counts, lo_usable, p, round_hyp, cap):
    """counts, status: [F, H] with H >= cap, as in ransac_adaptive_reference.simulate.  lo_counts, lo_usable: [F, rounds, n] -- the inlier
    count at thresh of the refit of scene f in step k of round r, and whether that refit is usable (status 0 or 2, fitted to >= 4); n = 0:
    no LO.  Every scene active in a round takes all n steps, finished by the round's own update or not.  Returns hyp_used, winner (the
    minimal hypothesis that seeded the running pose), best, lo_taken, certified [F], active (one int array of scene indices per round),
    done (per round, the flags in the order of its active list) and from_fit [F] (whether the running pose is a refit)."""
    counts, status, lo_counts, lo_usable = np.asarray(counts), np.asarray(status), np.asarray(lo_counts), np.asarray(lo_usable)
    F = counts.shape[0]
    assert counts.shape[1] >= cap and status.shape == counts.shape and len(sizes) == F and lo_counts.shape == lo_usable.shape
    n = lo_counts.shape[2] if lo_counts.ndim == 3 else 0
    hyp_used, winner, certified, lo_taken = (np.zeros(F, dtype=np.int64) for _ in range(4))
    best, from_fit = np.full(F, -1, dtype=np.int64), np.zeros(F, dtype=bool)
    active, rounds, dones, h0, r = np.arange(F), [], [], 0, 0
    while len(active) and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        rounds.append(active.copy())
        drawn = h0 + Hr
        done = {}
        for f in active:
            c = counts[f, h0:drawn]
            j = int(np.argmax(c))
            if c[j] > best[f]:                 # strictly greater: the running best, minimal or refitted, keeps a tie
                best[f], winner[f], from_fit[f] = c[j], h0 + j, False
            certified[f] += int((status[f, h0:drawn] == 0).sum())
            hyp_used[f] = drawn
            done[f] = bool(drawn >= cap or drawn >= needed(best[f], sizes[f], p))
        for k in range(n):
            for f in active:
                if lo_usable[f, r, k] and lo_counts[f, r, k] >= best[f]:
                    best[f], from_fit[f] = lo_counts[f, r, k], True
                    lo_taken[f] += 1
                done[f] = done[f] or bool(drawn >= cap or drawn >= needed(best[f], sizes[f], p))
        dones.append(np.array([done[f] for f in active], dtype=bool))
        active = np.array([f for f in active if not done[f]], dtype=np.int64)
        h0 += Hr
        r += 1
    return {"hyp_used": hyp_used, "winner": winner, "best": best, "lo_taken": lo_taken, "certified": certified, "active": rounds, "done": dones,
            "from_fit": from_fit}


def pack45(Q):
    """the upper triangle of a symmetric 9 x 9 matrix, row by row"""
    return np.array([Q[i, j] for i in range(9) for j in range(i, 9)])


def count_poses(x, X, K, R, t, status, thresh):
    """inlier counts of the poses (R, t)[h] over one scene; a status outside (0, 2) counts 0"""
    c = np.array([int(taken(x, X, K, R[h], t[h], thresh)[0].sum()) for h in range(len(R))], dtype=np.int64)
    return np.where(np.isin(status, (0, 2)), c, 0)


class SceneReplay:
    """One scene of the experiment: its draws are the device sampler's (synth.philox_minimal_sets(cap, M, 4, seed)), its minimal solves the
    host build's, solved round by round on demand and kept, so that the plain call and the LO call of a scene share them."""

    def __init__(self, scene, seed, cap, thresh, eps=1e-6, max_iters=100):
        import hostsim
        from cvxpnpl_amd import synth

        self.hs, self.x, self.X, self.K = hostsim, scene["scene_2d"], scene["scene_3d"], scene["K"]
        self.M, self.cap, self.thresh = len(self.x), cap, thresh
        self.idx = synth.philox_minimal_sets(cap, self.M, 4, seed)
        self.opts = dict(eps=eps, max_iters=max_iters)
        self.rounds = {}

    def round(self, h0, Hr):
        """(R, t, count) of hypotheses h0 .. h0 + Hr - 1"""
        if (h0, Hr) not in self.rounds:
            idx = self.idx[h0:h0 + Hr]
            sol = self.hs.solve_batch(self.x[idx], self.X[idx], None, None, self.K, self.hs.default_opts(**self.opts))
            self.rounds[(h0, Hr)] = (sol["R"], sol["t"], count_poses(self.x, self.X, self.K, sol["R"], sol["t"], sol["status"], self.thresh))
        return self.rounds[(h0, Hr)]

    def refit(self, R, t, thresh_k):
        """the LO solve of one step at the pose (R, t): (R, t, status, size of the set) -- status 3 when fewer than three are taken"""
        mask, _ = taken(self.x, self.X, self.K, R, t, thresh_k)
        cnt = int(mask.sum())
        if cnt < 3:
            return R, t, 3, cnt
        rc, B, Q = self.hs.assemble(self.x[mask], self.X[mask], None, None, self.K)
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
                n_new = int(taken(self.x, self.X, self.K, fR, ft, self.thresh)[0].sum())
                if take_fit(st, cnt, n_new, best):
                    best, pose, lo_taken = n_new, (fR, ft), lo_taken + 1
                done = done or drawn >= needed(best, self.M, p)
            h0, rounds = drawn, rounds + 1
            if done:
                break
        return {"hyp_used": h0, "best": best, "lo_taken": lo_taken, "rounds": rounds}
