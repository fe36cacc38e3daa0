"""What the tests of the scale estimate and the sandwich covariance share: the cases, each built with assertions made of the references
alone (tests/refine_robust_reference.py, tests/refine_robust_auto_reference.py), and the references' own results, computed once.

A case is tests/refine_robust_cases.py's dict.  The arrays are shared between the tests, which leave them unchanged.
"""
import functools

import numpy as np

import refine_robust_auto_reference as ar
import refine_robust_cases as cs
import refine_robust_reference as rr

HUBER_MARGIN = 1e-3  # no record within this relative distance of delta^2 under Huber: the reference's stencil must not cross the kink


def scale_cases():
    """clean and contaminated problems at their starting poses; the Cauchy ones carry weights (which the median ignores)"""
    return [cs.clean(n_p, n_l, loss) for n_p, n_l in cs.CLEAN_SHAPES for loss in ("huber", "cauchy")] + [cs.contaminated("huber")]


@functools.lru_cache(maxsize=None)
def masked():
    """the contaminated problems with every third point masked, every fourth line at weight 0 and one degenerate line (a = b): the records
    that are not live carry numbers that would spoil the median (NaN, 1e9)"""
    base = cs.contaminated("huber")
    kw = {k: v.copy() for k, v in base["kw"].items()}
    B = len(base["R0"])
    mp, wl = np.ones((B, 20), np.uint8), np.ones((B, 10))
    mp[:, ::3] = 0
    kw["pts_2d"][:, ::3] = np.nan
    kw["pts_3d"][:, ::3] = 1e9
    wl[:, ::4] = 0.0
    kw["line_3d"][:, ::4] = np.nan
    kw["line_2d"][:, 1, 1] = kw["line_2d"][:, 1, 0]
    kw.update(mask_pts=mp, weights_lines=wl)
    case = dict(base, name="masked", kw=kw)
    for b in range(B):
        lp, ll, *_ = rr.live_weights(**cs.one(case, b))
        assert lp.sum() == 13 and ll.sum() == 6
        assert ar.entry_status(case["K"][b], case["R0"][b], case["t0"][b], **cs.one(case, b)) == 0
    return case


@functools.lru_cache(maxsize=None)
def ties(m, split):
    """m point records that are copies of one record (split False: every s_k equal) or of two (split True: the lower ceil(m / 2) copies of
    A, the others of B with a larger s, so that for an even m the two middle values differ)."""
    base = cs.clean(10, 0, "huber")
    b = 0
    idx = [0] * m
    if split:
        s = rr.squares(base["K"][b], base["R0"][b], base["t0"][b], **cs.one(base, b))[0]
        lo, hi = (0, 1) if s[0] < s[1] else (1, 0)
        assert s[lo] < s[hi]
        idx = [lo] * ((m + 1) // 2) + [hi] * (m // 2)
    kw = {"pts_2d": base["kw"]["pts_2d"][b:b + 1, idx].copy(), "pts_3d": base["kw"]["pts_3d"][b:b + 1, idx].copy(), "line_2d": None, "line_3d": None}
    case = dict(base, name=f"ties-{m}-{split}", K=base["K"][b:b + 1], R0=base["R0"][b:b + 1], t0=base["t0"][b:b + 1], kw=kw)
    s = rr.squares(case["K"][0], case["R0"][0], case["t0"][0], **cs.one(case, 0))[0]
    assert len(s) == m and len(set(s.tolist())) == (2 if split else 1)
    if split and m % 2 == 0:
        ss = np.sort(s)
        assert ss[m // 2 - 1] != ss[m // 2]
    return case


COV_CASES = (("clean", 10, 0), ("clean", 5, 5), ("clean", 0, 6), ("contaminated", 20, 10))


def _cov_base(kind, n_p, n_l, loss):
    return cs.clean(n_p, n_l, loss) if kind == "clean" else cs.contaminated_checked()[loss]


@functools.lru_cache(maxsize=None)
def cov_case(kind, n_p, n_l, loss):
    """A case at the REFERENCE's minimum of its robust cost (tests/refine_robust_cases.py's reference runs), with the reference's sandwich
    covariance of every problem: (case with R0 / t0 replaced by the minimum, [(V, floor, H, B)]).  Asserted: the runs converged, no record
    within HUBER_MARGIN of delta^2 under Huber, every reference H positive definite."""
    base = _cov_base(kind, n_p, n_l, loss)
    runs = cs.reference_runs(base)
    R = np.stack([r["R"] for r in runs])
    t = np.stack([r["t"] for r in runs])
    case = dict(base, name=base["name"] + "-minimum", R0=R, t0=t)
    refs = []
    for b, r in enumerate(runs):
        assert r["status"] == 0, (case["name"], b, r["status"])
        one = cs.one(case, b)
        if loss == "huber":
            s = rr.squares(case["K"][b], R[b], t[b], **one)[0]
            assert (np.abs(s / case["delta"] ** 2 - 1.0) > HUBER_MARGIN).all(), (case["name"], b)
        V, floor, H, Bm = ar.sandwich(case["K"][b], R[b], t[b], loss, case["delta"], **one)
        assert (np.linalg.eigvalsh(H) > 0).all(), (case["name"], b)
        refs.append((V, floor, H, Bm))
    return case, refs


def pack_kwargs(case):
    """the keyword arguments of the library's host forms"""
    return {k: v for k, v in case["kw"].items() if v is not None}

