"""What the refinement tests share: the synthetic problems, their starts, the edge-case batch and the checks against
tests/refine_reference.py.  The bars are those of the issue that introduced the library: the reference's next step from a returned pose
is at most 1e-6 (the project's parity bar against its oracle), and the covariance agrees with the reference's normal equations to
1e3 cond(J^T J) eps, derived per problem."""
import functools

import numpy as np

import refine_reference as ref
from cvxpnpl_amd import synth

EPS = np.finfo(np.float64).eps
STEP_BAR = 1e-6
SHAPES = ((10, 0, 1.0), (5, 5, 1.0), (17, 0, 2.0), (33, 7, 1.0), (0, 6, 1.0), (4, 0, 1.0))  # the six over-determined shapes (n_p, n_l, sigma)


def problem(batch, n_p, n_l, sigma, seed=11, rot=0.05, rel_t=0.05):
    """synth.make_pnpl started `rot` rad and `rel_t` of t off the truth; returns (data dict, R0, t0, kw) with kw the correspondence
    arguments of refine_pose_batch(_host)."""
    d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=seed)
    rs = np.random.RandomState(seed + 1)
    ax = rs.normal(size=(batch, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    R0 = np.stack([ref.expm_so3(rot * a) @ R for a, R in zip(ax, d["R_gt"])])
    t0 = d["t_gt"] * (1.0 + rel_t * rs.uniform(-1.0, 1.0, size=(batch, 3)))
    kw = {"pts_2d": d["pts_2d"] if n_p else None, "pts_3d": d["pts_3d"] if n_p else None,
          "line_2d": d["line_2d"] if n_l else None, "line_3d": d["line_3d"] if n_l else None}
    return d, R0, t0, kw


def one(kw, b, **extra):
    """Problem b of a batch, as the keyword arguments of the reference."""
    out = {k: v[b] for k, v in kw.items() if v is not None}
    out.update(extra)
    return out


def _h(h, data):
    """h of the reference's differences: a number, or "far" for ref.far_h of the problem's own data."""
    return ref.far_h(**data) if h == "far" else h


def worst_next_step(K, R, t, kw, rows=None, masks=None, h=1e-3):
    """max over the problems of |step| the REFERENCE would take next from (R[b], t[b]) at lambda_0 (h: the reference's difference step,
    "far" for ref.far_h per problem)."""
    worst = 0.0
    for b in (range(len(R)) if rows is None else rows):
        extra = {} if masks is None else {k: v[b] for k, v in masks.items() if v is not None}
        Kb = K[b] if np.ndim(K) == 3 else K
        data = one(kw, b, **extra)
        d, _, _ = ref.lm_step(Kb, R[b], t[b], h=_h(h, data), **data)
        worst = max(worst, float(np.linalg.norm(d)))
    return worst


def worst_cov_ratio(K, out, kw, sigma_px=0.0, rows=None, h=1e-3):
    """max over the problems of |cov (J^T J_ref / sigma^2) - I|_max / (1e3 cond(J^T J_ref) eps): at most 1 when the bound holds."""
    worst = 0.0
    for b in (range(len(out.R)) if rows is None else rows):
        Kb = K[b] if np.ndim(K) == 3 else K
        data = one(kw, b)
        _, A, r = ref.lm_step(Kb, out.R[b], out.t[b], h=_h(h, data), **data)
        s2 = sigma_px**2 if sigma_px > 0 else out.cost[b, 1] / (len(r) - 6)
        E = out.cov[b] @ (A / s2) - np.eye(6)
        worst = max(worst, float(np.abs(E).max() / (1e3 * np.linalg.cond(A) * EPS)))
    return worst


def edge_batch():
    """One batch of (8 points, 4 lines) problems holding every pass-through case beside live ones.  Returns (K, R0, t0, kw, status_in,
    masks, expected status per problem)."""
    B = 12
    d, R0, t0, kw = problem(B, 8, 4, 1.0, seed=23)
    kw = {k: v.copy() for k, v in kw.items()}
    status_in = np.zeros(B, np.int32)
    mp, ml = np.ones((B, 8), np.uint8), np.ones((B, 4), np.uint8)
    expect = np.zeros(B, np.int32)
    R0[1, 0, 0] = np.nan                                         # a NaN pose
    expect[1] = 2
    R0[2, 1] = -R0[2, 1]                                         # a reflection
    expect[2] = 2
    status_in[3] = 1                                             # a status outside admit_mask (0x5)
    expect[3] = 2
    status_in[4] = 2                                             # ... and one inside it beside status 0
    mp[5, 2:] = 0                                                # 2 live correspondences
    ml[5] = 0
    expect[5] = 3
    Y = kw["pts_3d"][6, 0] @ R0[6].T                             # one live point behind the camera
    t0[6, 2] = -Y[2] - 0.1
    expect[6] = 4
    kw["line_2d"][7, 1, 1] = kw["line_2d"][7, 1, 0]              # a degenerate 2D line among good ones: not live, the rest refine
    t0[8] = np.inf                                               # a non-finite translation
    expect[8] = 2
    return d["K"], R0, t0, kw, status_in, {"mask_pts": mp, "mask_lines": ml}, expect


def check_edge_batch(out, R0, t0, expect):
    assert out.status.tolist() == expect.tolist(), (out.status, expect)
    for b in np.nonzero(expect >= 2)[0]:
        assert out.R[b].tobytes() == R0[b].tobytes() and out.t[b].tobytes() == t0[b].tobytes(), b   # bit for bit
        assert np.isnan(out.cost[b]).all() and out.iters[b] == 0, b
        if out.cov is not None:
            assert np.isnan(out.cov[b]).all(), b
    live = np.nonzero(expect < 2)[0]
    assert np.isfinite(out.R[live]).all() and np.isfinite(out.cost[live]).all()
    assert (out.cost[live, 1] <= out.cost[live, 0]).all()
    n_live = np.full(len(expect), 12)
    n_live[5], n_live[7] = 2, 11
    assert out.n_live.tolist() == n_live.tolist(), out.n_live


# ---- the hard paths of the schedule (tests/test_refine_hard_paths_{host,gpu}.py) ----

HARD_SHAPES = ((10, 0), (5, 5), (33, 7))
# either side of the kernel switches of cvxpnpl_refine_batch at 16, 32 and 64 correspondences: full register sets, a point / line split
# inside one lane's records, and 65 = the re-reading kernel with one record on a second pass
BOUNDARY_SHAPES = ((16, 0), (9, 7), (32, 0), (20, 12), (64, 0), (40, 24), (65, 0), (40, 25))
FAR_OFFSETS = (1e2, 1e4, 1e6)


@functools.lru_cache(maxsize=None)
def _hard_all():
    """The three hard-start batches with the reference's own run of each problem.  What makes them hard is asserted here, of the reference
    alone, so that the inputs cannot silently go easy: rejected trials, a trial with a record behind the camera, and convergence all the
    same."""
    out = {}
    for n_p, n_l in HARD_SHAPES:
        d, R0, t0, kw = problem(12, n_p, n_l, 1.0, seed=31, rot=1.5, rel_t=0.5)
        runs = [ref.refine(d["K"], R0[b], t0[b], max_iters=100, **one(kw, b)) for b in range(12)]
        out[(n_p, n_l)] = (d, R0, t0, kw, runs)
    runs = [r for v in out.values() for r in v[4]]
    assert sum(r["rejected"] > 0 for r in runs) >= 6, [r["rejected"] for r in runs]
    assert sum(r["behind_trials"] > 0 for r in runs) >= 1, [r["behind_trials"] for r in runs]
    assert all(r["status"] == 0 for r in runs), [r["status"] for r in runs]
    return out


def hard_starts(shape):
    """problem(12, n_p, n_l, 1.0, seed=31) started 1.5 rad and 50 % of t off the truth.  Returns (data, R0, t0, kw, the reference's run of
    every problem); the arrays are shared between the tests, which leave them unchanged."""
    return _hard_all()[tuple(shape)]


MIXED = {"ordinary": (0, 7), "nan_pose": (1,), "refined": (2,), "collinear": (3,), "coincident": (4,), "hard": (5, 9), "behind": (6,),
         "nan_2d": (8,), "inf_3d": (10,), "nan_3d": (11,)}


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """12 problems of 10 points, ordered so that each wavefront of four (0-3, 4-7, 8-11) holds unlike neighbours: problems that end after
    1 or 2 trials beside one that takes most of 100, and every pass-through beside live ones; the last four are three problems with a
    non-finite number in a live record and one hard start.  Returns (K, R0, t0, kw, expected statuses: a tuple of the allowed ones per
    problem); MIXED names the rows.  Shared: leave the arrays unchanged."""
    d, R0, t0, kw = problem(12, 10, 0, 1.0, seed=31)
    _, Rh, th, _, runs = hard_starts((10, 0))
    kw = {k: (None if v is None else v.copy()) for k, v in kw.items()}
    p2, p3 = kw["pts_2d"], kw["pts_3d"]
    R0, t0 = R0.copy(), t0.copy()
    expect = [(0,)] * 12
    rej = [b for b in range(12) if runs[b]["rejected"] > 0]
    assert len(rej) >= 2, rej
    # a hard start moves from its own row to a fixed one WITH its data, so that MIXED does not depend on which rows the reference rejects in
    for row, b in zip(MIXED["hard"], rej):
        p2[row], p3[row], R0[row], t0[row] = p2[b].copy(), p3[b].copy(), Rh[b], th[b]
    b = MIXED["collinear"][0]                                    # X_i on one line through the scene under the 2D data of the scattered points:
    p3[b] = p3[b].mean(0) + np.linspace(-0.5, 0.5, 10)[:, None] * np.array([0.6, -0.3, 0.5])   # no pose fits, the rotation about the line is free
    expect[b] = (0, 1)                                           # (most of 100 trials: the slow neighbour of its wavefront)
    b = MIXED["refined"][0]                                      # the reference's own minimum: nothing left to do
    r = ref.refine(d["K"], R0[b], t0[b], max_iters=100, **one(kw, b))
    assert r["status"] == 0
    R0[b], t0[b] = r["R"], r["t"]
    R0[MIXED["nan_pose"][0], 1, 2] = np.nan
    expect[MIXED["nan_pose"][0]] = (2,)
    # every 3D point the same: no rotation is observable and every Cholesky fails.  (Coordinates of a few bits, so that the mean of the ten is
    # the point itself: where the mean is rounded, X - c is 1e-17, not 0, the scaled damping makes that positive definite, and the run
    # spends max_iters trials on rotations of 1e15 rad about the point at an unchanged cost -- status 1, not 3.)
    b = MIXED["coincident"][0]
    p3[b] = np.array([0.25, -0.125, 0.5])
    expect[b] = (3,)
    b = MIXED["behind"][0]
    Y = p3[b, 3] @ R0[b].T
    t0[b, 2] = -Y[2] - 0.1
    expect[b] = (4,)
    p2[MIXED["nan_2d"][0], 4, 1] = np.nan
    p3[MIXED["inf_3d"][0], 9, 0] = np.inf
    p3[MIXED["nan_3d"][0], 0, 2] = np.nan
    for name in ("nan_2d", "inf_3d", "nan_3d"):
        expect[MIXED[name][0]] = (4,)
    return d["K"], R0, t0, kw, tuple(expect)


def far_scene(offset):
    """problem(12, 10, 0, 1.0, seed=31) with every 3D point shifted by o = offset (1, -2, 0.5) and the start t0 - R0 o: the same problems in
    the camera frame, far from the world origin.  offset 0 is the unshifted batch.  Returns (data, R0, t0, kw, o)."""
    d, R0, t0, kw = problem(12, 10, 0, 1.0, seed=31)
    o = offset * np.array([1.0, -2.0, 0.5])
    kw = dict(kw, pts_3d=kw["pts_3d"] + o)
    return d, R0, t0 - R0 @ o, kw, o


def boundary_masks(n_p, n_l, batch):
    """mask_pts / mask_lines that switch off every third record, counted through points then lines, the same in every problem."""
    keep = np.ones(n_p + n_l, np.uint8)
    keep[2::3] = 0
    return {"mask_pts": np.tile(keep[:n_p], (batch, 1)) if n_p else None, "mask_lines": np.tile(keep[n_p:], (batch, 1)) if n_l else None}


def spoil_masked(kw, masks):
    """A copy of the correspondences with the data of the masked-off records overwritten: NaN in the 2D half, 1e9 in the 3D half."""
    out = {k: (None if v is None else v.copy()) for k, v in kw.items()}
    for m, k2, k3 in (("mask_pts", "pts_2d", "pts_3d"), ("mask_lines", "line_2d", "line_3d")):
        if masks.get(m) is not None:
            off = masks[m] == 0
            out[k2][off] = np.nan
            out[k3][off] = 1e9
    return out


def compacted(kw, masks):
    """The live records alone (the masks are the same in every problem)."""
    out = {}
    for m, k2, k3 in (("mask_pts", "pts_2d", "pts_3d"), ("mask_lines", "line_2d", "line_3d")):
        if kw.get(k2) is None:
            out[k2] = out[k3] = None
            continue
        keep = np.ones(kw[k2].shape[1], bool) if masks.get(m) is None else masks[m][0] != 0
        out[k2], out[k3] = np.ascontiguousarray(kw[k2][:, keep]), np.ascontiguousarray(kw[k3][:, keep])
    return out


def check_mixed(out, R0, t0, expect):
    """What every path owes mixed_batch(): the statuses, the pass-through, and what the degenerate rows end as."""
    assert all(s in e for s, e in zip(out.status.tolist(), expect)), (out.status, expect)
    assert (out.n_live == 10).all()
    for b in range(12):
        if out.status[b] >= 2:
            assert out.R[b].tobytes() == R0[b].tobytes() and out.t[b].tobytes() == t0[b].tobytes(), b   # bit for bit
            assert np.isnan(out.cost[b]).all() and out.iters[b] == 0 and np.isnan(out.cov[b]).all(), b
        else:
            assert np.isfinite(out.R[b]).all() and np.isfinite(out.t[b]).all() and out.cost[b, 1] <= out.cost[b, 0], b
    b = MIXED["coincident"][0]
    assert out.status[b] == 3 and out.iters[b] == 0                                              # (16 internal trials, none with a factorisation)
    b = MIXED["collinear"][0]
    assert np.isnan(out.cov[b]).all()
    for b in MIXED["ordinary"] + MIXED["refined"] + MIXED["hard"]:
        assert np.isfinite(out.cov[b]).all(), b
    assert out.iters[MIXED["refined"][0]] <= 2


def check_far(out, base, d, kw, o, offset):
    """A run on far_scene(offset) against the run on the unshifted batch: the same problems in the camera frame."""
    assert out.status.tolist() == base.status.tolist() and (out.status == 0).all()
    assert out.iters.tolist() == base.iters.tolist()
    dR, dt = np.abs(out.R - base.R).max(), np.abs(out.R @ o + out.t - base.t).max()
    dc = (np.abs(out.cost - base.cost) / base.cost).max()
    nxt = worst_next_step(d["K"], out.R, out.t, kw, h="far")
    print(f"offset {offset:g}: R within {dR:.1e}, R o + t within {dt:.1e}, cost within {dc:.1e}, reference's next step (scaled h) <= {nxt:.1e}")
    assert dR <= STEP_BAR and dt <= STEP_BAR
    assert dc <= 1e-12 * max(1.0, np.linalg.norm(o))         # the rounding of X + o, eps |o| relative to a scene of unit size, with a margin of 100
    assert nxt <= STEP_BAR
    if offset <= 1e2:
        # (only here: beyond, cond(J^T J) in the PUBLIC chart -- the rotation moves points |o| away -- passes 1 / eps, the bound
        # 1e3 cond eps exceeds 1 and says nothing about the covariance)
        ratio = worst_cov_ratio(d["K"], out, kw, h="far")
        print(f"   covariance error / bound <= {ratio:.3f}")
        assert ratio <= 1.0
