"""What the tests of the robust refinement's backward pass share: small batches of synthetic problems AT the reference's own polished
minimum of the robust cost (tests/refine_robust_grad_reference.py), with random upstream gradients.  Every builder asserts, of the
reference alone, what the tests rely on:

- every problem is stationary to 1e-12 -- |g| <= 1e-12 sum omega |J||r| -- or the pose fits the data exactly (rms residual below 1e-10
  px: the minimal problems, 3 points or 3 lines, where g vanishes with r); the scenes shifted 1e4 from the origin, and only they, get
  the representability floor of the ratio instead (tests/refine_grad_cases.py);
- the full H -- rho'' term included -- is positive definite;
- under Huber and Cauchy at least one record has s_k > delta^2, so that the rho'' term is exercised.  (The minimal problems cannot:
  their fit is exact, every s_k is 0 to rounding; they are kept for the shapes' sake and the condition is asserted of every other case);
- under Huber every record has |sqrt(s_k) - delta| > 1e-3 delta: the derivative is one-sided at the kink, and the reference's and the
  library's sides must not differ;
- on the contaminated cases the reference's gradients with the rho'' term struck differ from the true ones by more than 1e-3 relative.

No problem is excluded: the seeds are ones for which all of that holds.  The results are cached and shared: leave the arrays unchanged."""
import functools

import numpy as np

import refine_grad_cases as gc
import refine_robust_cases as rbc
import refine_robust_grad_reference as rr

STATIONARY = 1e-12
EXACT_FIT_PX = 1e-10
KINK = 1e-3
CLEAN_DELTA = 1.0
ROBUST = ("huber", "cauchy")

# the clean shapes of tests/refine_grad_cases.py at sigma = 1 px: (n_p, n_l, batch, seed, options); each runs under Huber and Cauchy
SHAPES = {
    "pnp3": (3, 0, 2, 402, {}), "pnp6": (6, 0, 2, 404, {}), "pnp10": (10, 0, 2, 406, {}),
    "pnl3": (0, 3, 2, 407, {}), "pnl6": (0, 6, 2, 410, {}), "pnpl5+5": (5, 5, 2, 412, {}),
    "pnp10-Kper": (10, 0, 2, 413, {"K_per": True}), "pnpl5+5-far": (5, 5, 2, 416, {"far": True}),
}
CLEAN = tuple(f"{n}-{loss}" for n in SHAPES for loss in ROBUST)
CONTAMINATED = tuple(f"contaminated-{loss}" for loss in ROBUST)
ALL = CLEAN + CONTAMINATED


def one(c, b, weights=True):
    """Problem b of a case, as the keyword arguments of the reference."""
    out = {k: v[b] for k, v in c["kw"].items() if v is not None}
    if weights:
        out.update({k: v[b] for k, v in c["w"].items() if v is not None})
    return out


def K_of(K, b):
    return K[b] if np.ndim(K) == 3 else K


def is_minimal(c):
    kw = c["kw"]
    return sum(v.shape[1] for k, v in kw.items() if v is not None and k.endswith("3d")) == 3


def _checked(name, c, far=False):
    """The reference's own claims about a case (see the module's docstring)."""
    loss, delta = c["loss"], c["delta"]
    any_above = False
    for b in range(len(c["R"])):
        K = K_of(c["K"], b)
        rel, rms, ev, floor = rr.stationarity(c["R"][b], c["t"][b], K, loss, delta, **one(c, b))
        assert rel <= max(STATIONARY, floor if far else 0.0) or rms <= EXACT_FIT_PX, (name, b, rel, rms, floor)
        assert ev > 0.0, (name, b, ev)
        root = np.sqrt(rr.squares(c["R"][b], c["t"][b], K, **one(c, b, weights=False)))
        any_above = any_above or bool((root > delta).any())
        if loss == "huber":
            assert (np.abs(root - delta) > KINK * delta).all(), (name, b, root)
    assert any_above or is_minimal(c), name
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """{"K", "R", "t", "kw", "w", "GR", "gt", "loss", "delta"} of a named case."""
    if name in CONTAMINATED:
        return _contaminated(name.split("-")[1])
    shape, loss = name.rsplit("-", 1)
    n_p, n_l, batch, seed, opt = SHAPES[shape]
    K, R0, t0, kw = gc.polished_batch(batch, n_p, n_l, 1.0, seed, **opt)   # the data, and the least-squares minimum as a start
    rs = np.random.RandomState(seed + 29)
    w = {"weights_pts": rs.uniform(0.25, 4.0, (batch, n_p)) if n_p else None, "weights_lines": rs.uniform(0.25, 4.0, (batch, n_l)) if n_l else None}
    c = {"K": K, "kw": kw, "w": w, "loss": loss, "delta": CLEAN_DELTA, "GR": rs.normal(size=(batch, 3, 3)), "gt": rs.normal(size=(batch, 3))}
    c["R"], c["t"] = np.empty_like(R0), np.empty_like(t0)
    for b in range(batch):
        c["R"][b], c["t"][b] = rr.polish(R0[b], t0[b], K_of(K, b), loss, CLEAN_DELTA, **one(c, b))
    return _checked(name, c, far=opt.get("far", False))


def _contaminated(loss):
    """tests/refine_robust_cases.py's contaminated data (20 points + 10 lines, sigma = 0.5 px, 30 % displaced by 20-200 px, delta = 2 px),
    no weights, polished by the reference from the true pose."""
    src = rbc.contaminated(loss)
    B = len(src["R_gt"])
    kw = {k: src["kw"][k] for k in ("pts_2d", "pts_3d", "line_2d", "line_3d")}
    rs = np.random.RandomState(97)
    c = {"K": src["K"], "kw": kw, "w": {"weights_pts": None, "weights_lines": None}, "loss": loss, "delta": src["delta"],
         "GR": rs.normal(size=(B, 3, 3)), "gt": rs.normal(size=(B, 3)), "displaced": src["displaced"]}
    c["R"], c["t"] = np.empty_like(src["R_gt"]), np.empty_like(src["t_gt"])
    for b in range(B):
        c["R"][b], c["t"][b] = rr.polish(src["R_gt"][b], src["t_gt"][b], c["K"][b], loss, c["delta"], **one(c, b))
    _checked(f"contaminated-{loss}", c)
    for b in range(B):   # the rho'' term is not a detail here
        args = (c["R"][b], c["t"][b], c["K"][b], loss, c["delta"], c["GR"][b], c["gt"][b])
        full, struck = rr.flat(rr.reference_vjp(*args, **one(c, b))), rr.flat(rr.reference_vjp(*args, variant="struck", **one(c, b)))
        assert rr.rel_err(struck, full) > 1e-3, (loss, b, rr.rel_err(struck, full))
    return c


@functools.lru_cache(maxsize=None)
def saddle():
    """tests/refine_grad_cases.py's noisy 3-line problem under the Cauchy loss at delta = 1 px: Newton's method ends at a stationary point
    of the robust cost whose full H has a negative eigenvalue.  A case dict of batch 1, no weights."""
    s = gc.saddle()
    c = dict(s, w={"weights_pts": None, "weights_lines": None}, loss="cauchy", delta=1.0)
    R, t = rr.polish(s["R"][0], s["t"][0], s["K"], "cauchy", 1.0, iters=100, pure=True, **one(c, 0))
    c["R"], c["t"] = R[None], t[None]
    rel, rms, ev, _ = rr.stationarity(R, t, s["K"], "cauchy", 1.0, **one(c, 0))
    assert (rel <= STATIONARY or rms <= EXACT_FIT_PX) and ev < -1e-4, (rel, rms, ev)
    return c


def shaped(n_p, n_l, batch, seed=41, sigma=1.0, weights=True):
    """A batch of any shape for the device-against-host tests, which refine it themselves: tests/refine_grad_cases.py's shaped() plus
    weights uniform in [0.25, 4].  Returns (K, R, t, kw, w, GR, gt)."""
    K, R, t, kw, GR, gt = gc.shaped(n_p, n_l, batch, seed, sigma)
    rs = np.random.RandomState(seed + 11)
    w = {"weights_pts": rs.uniform(0.25, 4.0, (batch, n_p)) if n_p and weights else None,
         "weights_lines": rs.uniform(0.25, 4.0, (batch, n_l)) if n_l and weights else None}
    return K, R, t, kw, w, GR, gt
