"""What the robust-refinement tests share: the cases, each built with an assertion -- made of the reference alone
(tests/refine_robust_reference.py) -- of what makes it the case it claims to be, and the reference's own run of every problem.

A case is a dict: name, K [B,3,3] (a camera per problem), R0, t0, kw (the correspondence arguments, with weights_pts / weights_lines /
mask_pts / mask_lines where the case has them), loss, delta, and whatever the case knows about itself (R_gt, t_gt, displaced).  The arrays
are shared between the tests, which leave them unchanged.
"""
import functools

import numpy as np

import refine_cases as rc
import refine_reference as ref
import refine_robust_reference as rr
from cvxpnpl_amd import synth

MAX_ITERS = 100
CLEAN_SHAPES = ((3, 0), (6, 0), (10, 0), (0, 3), (0, 6), (5, 5))
CLEAN_DELTA = 1.0  # at sigma = 1 px a good part of the records sits on each branch of the Huber loss


def one(case, b):
    """Problem b of a case, as the keyword arguments of the reference."""
    return {k: v[b] for k, v in case["kw"].items() if v is not None}


def own_cameras(d, kw, batch, seed):
    """A camera per problem: K_b = A_b K with A_b a scaling about a shifted origin, and every 2D sample mapped by A_b (exactly the same
    scene seen by another camera; the pixel noise scales with it)."""
    rs = np.random.RandomState(seed)
    s, c = rs.uniform(0.8, 1.3, batch), rs.uniform(-30.0, 30.0, (batch, 2))
    K = np.zeros((batch, 3, 3))
    out = dict(kw)
    for b in range(batch):
        A = np.array([[s[b], 0.0, c[b, 0]], [0.0, s[b], c[b, 1]], [0.0, 0.0, 1.0]])
        K[b] = A @ d["K"]
    for k in ("pts_2d", "line_2d"):
        if kw.get(k) is not None:
            sh = (batch,) + (1,) * (kw[k].ndim - 2)
            out[k] = kw[k] * s.reshape(sh + (1,)) + c.reshape(sh + (2,))
    return K, out


@functools.lru_cache(maxsize=None)
def clean(n_p, n_l, loss):
    """(a) two problems at sigma = 1 px, started 0.05 rad and 5 % of t off the truth; under the Cauchy loss with random weights in [0.1, 2]."""
    B = 2
    d, R0, t0, kw = rc.problem(B, n_p, n_l, 1.0, seed=41 + n_p + 3 * n_l)
    K, kw = own_cameras(d, kw, B, seed=7)
    if loss == "cauchy":
        rs = np.random.RandomState(3)
        kw["weights_pts"] = rs.uniform(0.1, 2.0, (B, n_p)) if n_p else None
        kw["weights_lines"] = rs.uniform(0.1, 2.0, (B, n_l)) if n_l else None
    return {"name": f"clean-{n_p}-{n_l}-{loss}", "K": K, "R0": R0, "t0": t0, "kw": kw, "loss": loss, "delta": CLEAN_DELTA, "R_gt": d["R_gt"],
            "t_gt": d["t_gt"], "minimal": 2 * (n_p + n_l) == 6}


def pose_distance(R, t, R_gt, t_gt):
    return float(synth.geodesic(R, R_gt) + np.linalg.norm(t - t_gt) / np.linalg.norm(t_gt))


CONTAMINATED_B, CONTAMINATED_SEED = 3, 61


@functools.lru_cache(maxsize=None)
def _contaminated_data():
    B = CONTAMINATED_B
    d, R0, t0, kw = rc.problem(B, 20, 10, 0.5, seed=CONTAMINATED_SEED)
    kw = {k: v.copy() for k, v in kw.items()}
    rs = np.random.RandomState(CONTAMINATED_SEED + 5)
    displaced = np.zeros((B, 30), bool)
    for b in range(B):
        ip, il = rs.choice(20, 6, replace=False), rs.choice(10, 3, replace=False)
        displaced[b, ip] = True
        displaced[b, 20 + il] = True
        for idx, key, per in ((ip, "pts_2d", 1), (il, "line_2d", 2)):     # every displaced 2D sample by 20-200 px in a direction of its own
            n = len(idx) * per
            ang, mag = rs.uniform(0.0, 2.0 * np.pi, n), rs.uniform(20.0, 200.0, n)
            sh = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
            kw[key][b, idx] += sh.reshape(kw[key][b, idx].shape)
    return d, R0, t0, kw, displaced


@functools.lru_cache(maxsize=None)
def contaminated(loss):
    """(b) 20 points + 10 lines at sigma = 0.5 px, 30 % of the records (6 points, 3 lines) with their 2D samples displaced by 20-200 px,
    delta = 2 px, started 0.05 rad / 5 % off.  (sigma = 0.5: at delta = 2 a clean record then has rho' > 0.5 under both losses with
    probability 1 - e^-8; the issue leaves the noise of this case open.  One camera: the displacements and delta are in its pixels.)"""
    d, R0, t0, kw, displaced = _contaminated_data()
    return {"name": f"contaminated-{loss}", "K": np.tile(d["K"], (CONTAMINATED_B, 1, 1)), "R0": R0, "t0": t0, "kw": kw, "loss": loss, "delta": 2.0,
            "R_gt": d["R_gt"], "t_gt": d["t_gt"], "displaced": displaced, "minimal": False}


@functools.lru_cache(maxsize=None)
def exact_zero(loss):
    """(c) a record whose s_k is EXACTLY 0 at the start: R0 = I, t0 = (0, 0, 4), 3D points on a 1/8 grid whose mean is on the grid too, an
    integer camera, and record 0 at depth 4 -- every operation of its projection is exact in any order, so its residual is 0.0, not
    1e-17, and rho' is taken at s = 0 (the Huber inlier branch must not divide).  The other seven points carry the truth's projections plus
    noise, so the pose moves."""
    K = np.array([[512.0, 0.0, 320.0], [0.0, 512.0, 240.0], [0.0, 0.0, 1.0]])
    X = np.array([[0.25, -0.5, 0.0], [-0.5, 0.25, 0.5], [0.5, 0.5, -0.25], [-0.25, -0.25, 0.25], [0.375, -0.125, -0.5], [-0.375, 0.5, 0.125],
                  [0.125, -0.375, 0.375], [-0.125, 0.0, -0.5]])
    assert np.all(X.sum(0) * 8 == np.round(X.sum(0) * 8))
    R0, t0 = np.eye(3), np.array([0.0, 0.0, 4.0])
    R_gt, t_gt = ref.expm_so3(np.array([0.02, -0.03, 0.01])), np.array([0.02, -0.01, 4.1])
    rs = np.random.RandomState(77)
    h = (X @ R_gt.T + t_gt) @ K.T
    x = h[:, :2] / h[:, 2:] + rs.normal(0.0, 1.0, (8, 2))
    x[0] = [352.0, 176.0]                                         # K (X_0 + t0) / 4, exactly
    kw = {"pts_2d": x[None].copy(), "pts_3d": X[None].copy(), "line_2d": None, "line_3d": None}
    case = {"name": f"exact-zero-{loss}", "K": K[None].copy(), "R0": R0[None].copy(), "t0": t0[None].copy(), "kw": kw, "loss": loss, "delta": 1.0,
            "minimal": False}
    s = rr.squares(K, R0, t0, **one(case, 0))[0]
    assert s[0] == 0.0 and (s[1:] > 0).all(), s
    assert rr.rho_prime(loss, s, 1.0)[0] == 1.0
    return case


@functools.lru_cache(maxsize=None)
def all_outliers(loss):
    """(c) every record beyond delta at the start: the clean 10-point problems at delta = 1 px, started 0.05 rad off (a few pixels each)."""
    base = clean(10, 0, "huber")
    case = dict(base, name=f"all-outliers-{loss}", loss=loss, delta=1.0)
    for b in range(len(case["R0"])):
        s = rr.squares(case["K"][b], case["R0"][b], case["t0"][b], **one(case, b))[0]
        assert (s > 1.0).all(), s
    return case


@functools.lru_cache(maxsize=None)
def huge_delta():
    """(c) delta = 1e4 px: no record ever leaves the quadratic branch (the image is a few hundred pixels wide), Huber is L2."""
    base = clean(5, 5, "huber")
    case = dict(base, name="huge-delta", loss="huber", delta=1e4)
    for b in range(len(case["R0"])):
        s = rr.squares(case["K"][b], case["R0"][b], case["t0"][b], **one(case, b))[0]
        assert (s < 1e6).all(), s
    return case


def all_cases():
    out = [clean(n_p, n_l, loss) for n_p, n_l in CLEAN_SHAPES for loss in rr.LOSSES]
    out += [contaminated(loss) for loss in rr.LOSSES]
    out += [exact_zero("huber"), exact_zero("cauchy"), all_outliers("huber"), all_outliers("cauchy"), huge_delta()]
    return out


@functools.lru_cache(maxsize=None)
def _reference_runs(name):
    case = {c["name"]: c for c in all_cases()}[name]
    return tuple(rr.refine(case["K"][b], case["R0"][b], case["t0"][b], loss=case["loss"], delta=case["delta"], max_iters=MAX_ITERS, **one(case, b))
                 for b in range(len(case["R0"])))


def reference_runs(case):
    """The reference's run of every problem of a case (computed once)."""
    return _reference_runs(case["name"])


@functools.lru_cache(maxsize=None)
def contaminated_checked():
    """The three contaminated cases after the assertions that make them what they claim, on the reference alone: all three runs converge,
    the Huber and the Cauchy minimum are each at least 10x closer to the true pose than the L2 minimum, and at the robust minima rho' is
    below 0.5 on every displaced record and above 0.5 on every other."""
    cases = {loss: contaminated(loss) for loss in rr.LOSSES}
    runs = {loss: reference_runs(c) for loss, c in cases.items()}
    for b in range(CONTAMINATED_B):
        dist = {}
        for loss, c in cases.items():
            r = runs[loss][b]
            assert r["status"] == 0, (loss, b, r["status"], r["iters"])
            dist[loss] = pose_distance(r["R"], r["t"], c["R_gt"][b], c["t_gt"][b])
        assert dist["huber"] * 10.0 <= dist["l2"] and dist["cauchy"] * 10.0 <= dist["l2"], (b, dist)
        for loss in ("huber", "cauchy"):
            c, r = cases[loss], runs[loss][b]
            w, _, s = rr.robust_w_full(c["K"][b], r["R"], r["t"], loss, c["delta"], **one(c, b))
            assert (w[c["displaced"][b]] < 0.5).all() and (w[~c["displaced"][b]] > 0.5).all(), (loss, b, w)
    return cases
