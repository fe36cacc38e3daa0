"""What the tests of the refinement's backward pass share: small batches of synthetic problems AT the reference's own polished minimum,
with random upstream gradients.  Every builder asserts, of the reference (tests/refine_grad_reference.py) alone, what the tests rely on:
every problem it hands out is stationary to 1e-12 -- |g| <= 1e-12 sum |J||rho|, or the pose fits the data exactly (rms residual below
1e-10 px: noise-free data and the minimal problems, where g vanishes with rho and the ratio is 0 / 0) -- and has a positive definite
full Hessian.  For the scenes shifted 1e4 from the origin, and only there, the bar is the representability floor of the ratio instead
(rg.stationarity: t is stored to eps |t| = 2e-12, which alone moves g by eps |t| |H|, a few 1e-11 of the scale): no pose in float64
does better, and it is asserted that every other case's floor is below 1e-12.  No problem is excluded: the seeds are ones for which that holds.  The results are cached and shared: leave the arrays
unchanged."""
import functools

import numpy as np

import refine_grad_reference as rg
from cvxpnpl_amd import synth

STATIONARY = 1e-12
EXACT_FIT_PX = 1e-10
FAR = 1e4 * np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])  # the far scene: shifted 1e4 from the origin

# name: (n_p, n_l, sigma, batch, seed, options)
CASES = {
    "pnp3-s0": (3, 0, 0.0, 3, 201, {}), "pnp3-s1": (3, 0, 1.0, 3, 202, {}),
    "pnp6-s0": (6, 0, 0.0, 3, 203, {}), "pnp6-s1": (6, 0, 1.0, 3, 204, {}),
    "pnp10-s0": (10, 0, 0.0, 3, 205, {}), "pnp10-s1": (10, 0, 1.0, 3, 206, {}),
    "pnl3-s0": (0, 3, 0.0, 3, 207, {}), "pnl3-s1": (0, 3, 1.0, 3, 307, {}),
    "pnl6-s0": (0, 6, 0.0, 3, 209, {}), "pnl6-s1": (0, 6, 1.0, 3, 210, {}),
    "pnpl5+5-s0": (5, 5, 0.0, 3, 211, {}), "pnpl5+5-s1": (5, 5, 1.0, 3, 212, {}),
    "pnp10-Kper": (10, 0, 1.0, 3, 213, {"K_per": True}), "pnpl5+5-Kper": (5, 5, 1.0, 3, 214, {"K_per": True}),
    "pnp10-far": (10, 0, 1.0, 3, 215, {"far": True}), "pnpl5+5-far": (5, 5, 1.0, 3, 216, {"far": True}),
}
NOISY = tuple(n for n, c in CASES.items() if c[2] > 0 and c[0] + c[1] > 3)   # over-determined with noise: where Gauss-Newton is wrong


def one(kw, b):
    """Problem b of a batch, as the keyword arguments of the reference."""
    return {k: v[b] for k, v in kw.items() if v is not None}


def K_of(K, b):
    return K[b] if np.ndim(K) == 3 else K


def polished_batch(batch, n_p, n_l, sigma, seed, K_per=False, far=False):
    """synth.make_pnpl polished by the reference from the ground truth.  Returns (K, R, t, kw) with kw the correspondence arguments."""
    d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=seed)
    rs = np.random.RandomState(seed + 7)
    K = d["K"]
    kw = {"pts_2d": d["pts_2d"] if n_p else None, "pts_3d": d["pts_3d"] if n_p else None,
          "line_2d": d["line_2d"] if n_l else None, "line_3d": d["line_3d"] if n_l else None}
    R0, t0 = d["R_gt"], d["t_gt"]
    if K_per:   # a camera of its own per problem: focal lengths, skew and centre moved, the images drawn again through it
        K = np.tile(K, (batch, 1, 1))
        K[:, 0, 0] *= rs.uniform(0.8, 1.25, batch)
        K[:, 1, 1] *= rs.uniform(0.8, 1.25, batch)
        K[:, 0, 1] = rs.uniform(-3.0, 3.0, batch)
        K[:, :2, 2] += rs.uniform(-20.0, 20.0, (batch, 2))
        for b in range(batch):
            if n_p:
                kw["pts_2d"][b] = synth.project(kw["pts_3d"][b][None], K[b], R0[b][None], t0[b][None])[0] + rs.normal(scale=sigma, size=(n_p, 2))
            if n_l:
                x = synth.project(kw["line_3d"][b].reshape(1, -1, 3), K[b], R0[b][None], t0[b][None])[0] + rs.normal(scale=sigma, size=(2 * n_l, 2))
                kw["line_2d"][b] = x.reshape(n_l, 2, 2)
    if far:     # the same images, the world origin moved far from the scene
        kw = {k: (v + FAR if v is not None and k.endswith("3d") else v) for k, v in kw.items()}
        t0 = t0 - R0 @ FAR
    R, t = np.empty_like(R0), np.empty_like(t0)
    for b in range(batch):
        R[b], t[b] = rg.polish(R0[b], t0[b], K_of(K, b), **one(kw, b))
    return K, R, t, kw


@functools.lru_cache(maxsize=None)
def case(name):
    """{"K", "R", "t", "kw", "GR", "gt"} of a named case; asserts the reference's own claims about it."""
    n_p, n_l, sigma, batch, seed, opt = CASES[name]
    K, R, t, kw = polished_batch(batch, n_p, n_l, sigma, seed, **opt)
    for b in range(batch):
        rel, rms, ev, floor = rg.stationarity(R[b], t[b], K_of(K, b), **one(kw, b))
        assert rel <= max(STATIONARY, floor) or rms <= EXACT_FIT_PX, (name, b, rel, rms, floor)
        assert floor <= STATIONARY or rms <= EXACT_FIT_PX or opt.get("far"), (name, b, floor)
        assert ev > 0.0, (name, b, ev)
    rs = np.random.RandomState(seed + 13)
    return {"K": K, "R": R, "t": t, "kw": kw, "GR": rs.normal(size=(batch, 3, 3)), "gt": rs.normal(size=(batch, 3))}


@functools.lru_cache(maxsize=None)
def saddle():
    """One noisy 3-line problem on which Newton's method from the ground truth ends at a stationary point that is NOT a minimum: the
    reference's full H has a negative eigenvalue there.  Returns a case dict of batch 1."""
    K, R, t, kw = polished_batch(3, 0, 3, 1.0, 322)
    b = 1
    rel, rms, ev, _ = rg.stationarity(R[b], t[b], K, **one(kw, b))
    assert rel <= STATIONARY and ev < -1e-4, (rel, rms, ev)
    rs = np.random.RandomState(5)
    return {"K": K, "R": R[b:b + 1], "t": t[b:b + 1], "kw": {k: (None if v is None else v[b:b + 1]) for k, v in kw.items()},
            "GR": rs.normal(size=(1, 3, 3)), "gt": rs.normal(size=(1, 3))}


@functools.lru_cache(maxsize=None)
def masked_case(name="pnpl5+5-s1"):
    """A case with every third record (counted through points then lines) switched off.  Returns (case polished on the LIVE records,
    masks, the compacted correspondences)."""
    n_p, n_l, sigma, batch, seed, opt = CASES[name]
    n_p, n_l = n_p + 3, n_l + 3                                      # so that the live records still over-determine the pose
    d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=seed + 100)
    kw = {"pts_2d": d["pts_2d"], "pts_3d": d["pts_3d"], "line_2d": d["line_2d"], "line_3d": d["line_3d"]}
    keep = np.ones(n_p + n_l, np.uint8)
    keep[2::3] = 0
    masks = {"mask_pts": np.tile(keep[:n_p], (batch, 1)), "mask_lines": np.tile(keep[n_p:], (batch, 1))}
    live = {"pts_2d": np.ascontiguousarray(kw["pts_2d"][:, keep[:n_p] != 0]), "pts_3d": np.ascontiguousarray(kw["pts_3d"][:, keep[:n_p] != 0]),
            "line_2d": np.ascontiguousarray(kw["line_2d"][:, keep[n_p:] != 0]), "line_3d": np.ascontiguousarray(kw["line_3d"][:, keep[n_p:] != 0])}
    R, t = np.empty_like(d["R_gt"]), np.empty_like(d["t_gt"])
    for b in range(batch):
        R[b], t[b] = rg.polish(d["R_gt"][b], d["t_gt"][b], d["K"], **one(live, b))
        rel, rms, ev, _ = rg.stationarity(R[b], t[b], d["K"], **one(live, b))
        assert (rel <= STATIONARY or rms <= EXACT_FIT_PX) and ev > 0.0, (name, b, rel, rms, ev)
    rs = np.random.RandomState(seed + 113)
    c = {"K": d["K"], "R": R, "t": t, "kw": kw, "GR": rs.normal(size=(batch, 3, 3)), "gt": rs.normal(size=(batch, 3))}
    return c, masks, live


def spoiled(kw, masks):
    """A copy of the correspondences with the masked-off records overwritten: NaN in the 2D half, 1e9 in the 3D half."""
    out = {k: (None if v is None else v.copy()) for k, v in kw.items()}
    for m, k2, k3 in (("mask_pts", "pts_2d", "pts_3d"), ("mask_lines", "line_2d", "line_3d")):
        if masks.get(m) is not None and out.get(k2) is not None:
            off = masks[m] == 0
            out[k2][off] = np.nan
            out[k3][off] = 1e9
    return out


def shaped(n_p, n_l, batch, seed=41, sigma=1.0):
    """A batch of any shape for the device-against-host tests, which refine it themselves (both paths run the same source at the same
    pose): the data, the ground-truth poses as a start, and random upstream gradients.  Returns (K, R, t, kw, GR, gt)."""
    d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=seed)
    kw = {"pts_2d": d["pts_2d"] if n_p else None, "pts_3d": d["pts_3d"] if n_p else None,
          "line_2d": d["line_2d"] if n_l else None, "line_3d": d["line_3d"] if n_l else None}
    rs = np.random.RandomState(seed + 3)
    return d["K"], d["R_gt"], d["t_gt"], kw, rs.normal(size=(batch, 3, 3)), rs.normal(size=(batch, 3))
