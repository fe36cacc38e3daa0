"""The host path of the robust refinement's backward pass (cvxpnpl_refine_robust_vjp_batch_host; csrc/refine_robust_vjp_core.h, the
source of the kernels) against an independent float64 autograd reference (tests/refine_robust_grad_reference.py: the residuals'
definition, torch.matrix_exp, rho from DESIGN.md section 17's table, rho' and rho'' by autograd, double backward) at the reference's
own polished minima of the robust cost (tests/refine_robust_grad_cases.py) -- no GPU.

Error: relative L2 per problem over all six gradients.  BOUND = 1e-10 (tests/test_refine_grad_host.py's); where the reference's own
floor (centred against plain chart) is above 1e-12 for a problem -- the two scenes shifted 1e4 from the origin, floors 3.7e-7 .. 3.0e-6
-- the bar is 100 x that floor.  Measured over the 18 cases: worst host-vs-reference error 1.6e-13 away from the far scenes
(pnp10-cauchy), 6.9e-10 on them (pnpl5+5-far-cauchy, floor 3.0e-6).

The rho'' term: on the contaminated cases the host path's distance to the reference WITHOUT the rho'' term is at least 1e3 x its
distance to the full one (measured: 2.1e12 x at the least, the gradients without the term being off by 1.4e-2 .. 1.4e-1 relative).

Finite differences of the reference's polished minimiser: central differences of <G_R, R*> + <g_t, t*> over every input coordinate and
every weight, R*, t* the reference's own Newton-polished minimiser of the perturbed data, against the host VJP at the base minimiser.
Steps 1e-4 px, 1e-6 scene units, 1e-4 of weight: below the cases' Huber kink margin (1e-3 px), so that no record changes branch.  Bar
1e-2 (tests/test_refine_grad_host.py's).  Measured: 2.0e-9 (10 points, Huber), 4.2e-10 (5 + 5, Huber), 1.3e-7 (10 points, Cauchy), 1.9e-8 (5 + 5, Cauchy).

End to end through the forward: the same differences through refine_pose_batch_robust_host at its default options (max_iters 30,
step_tol 1e-10), VJP at the pose the forward returns.  The forward stops at ~1e-7 relative stationarity, so the
differences carry its convergence error.  Steps 1e-3 px, 1e-5 scene units, 1e-3 of weight.  Measured: 1.3e-3 (10 points, Huber), 8.9e-5 (5 + 5, Huber),
8.4e-3 (10 points, Cauchy: two of its 120 perturbed problems stop at max_iters), 9.9e-4 (5 + 5, Cauchy); E2E_BAR = 8.4e-2 is 10 x the worst.
"""
import numpy as np
import pytest

import refine_grad_cases as gc
import refine_robust_grad_cases as rc
import refine_robust_grad_reference as rr
from cvxpnpl_amd.refine_grad import refine_vjp_host
from cvxpnpl_amd.refine_robust import refine_pose_batch_robust_host
from cvxpnpl_amd.refine_robust_grad import refine_vjp_robust_host

BOUND = 1e-10
FLOOR_SMALL = 1e-12
FD_BAR = 1e-2
E2E_BAR = 8.4e-2
CORR = rr.NAMES[:4]
WGT = rr.NAMES[4:]


def host(c, **kw):
    args = dict(K=c["K"], loss=c["loss"], scale_px=c["delta"], **c["kw"], **c["w"])
    args.update(kw)
    return refine_vjp_robust_host(c["R"], c["t"], args.pop("status", None), args.pop("grad_R", c["GR"]), args.pop("grad_t", c["gt"]), **args)


def all_zero(out, b=None):
    return all(not np.any(v if b is None else v[b]) for k, v in out.items() if k in rr.NAMES and v is not None)


def ref_args(c, b):
    return (c["R"][b], c["t"][b], rc.K_of(c["K"], b), c["loss"], c["delta"], c["GR"][b], c["gt"][b])


@pytest.mark.parametrize("name", rc.ALL)
def test_host_matches_the_autograd_reference(name):
    c = rc.case(name)
    out = host(c)
    for b in range(len(c["R"])):
        assert out["vjp_status"][b] == 0, (name, b, out["vjp_status"])
        truth, floor = rr.truth_and_floor(*ref_args(c, b), **rc.one(c, b))
        err = rr.rel_err(rr.flat(out, b), truth)
        bar = BOUND if floor <= FLOOR_SMALL else 100.0 * floor
        print(f"{name}[{b}]: host-vs-reference {err:.2e}, floor (plain chart) {floor:.2e}, bar {bar:.1e}, info {out['info'][b]}")
        assert err < bar, (name, b, err, floor)


@pytest.mark.parametrize("name", rc.CONTAMINATED)
def test_the_hessian_holds_the_second_derivative_of_the_loss(name):
    c = rc.case(name)
    out = host(c)
    for b in range(len(c["R"])):
        full = rr.flat(rr.reference_vjp(*ref_args(c, b), **rc.one(c, b)))
        struck = rr.flat(rr.reference_vjp(*ref_args(c, b), variant="struck", **rc.one(c, b)))
        got = rr.flat(out, b)
        d_full, d_struck = rr.rel_err(got, full), rr.rel_err(got, struck)
        print(f"{name}[{b}]: to the full reference {d_full:.2e}, to the one without rho'' {d_struck:.2e}, ratio {d_struck / d_full:.1e}")
        assert d_struck >= 1e3 * d_full and d_struck > 1e-3, (name, b, d_full, d_struck)


STEPS = {"pts_2d": 1e-4, "line_2d": 1e-4, "pts_3d": 1e-6, "line_3d": 1e-6, "weights_pts": 1e-4, "weights_lines": 1e-4}


def _perturbations(c, b, steps):
    """[(name, flat index, signed copy of problem b's arguments)] for every input coordinate and every weight, + then -."""
    base = rc.one(c, b)
    out = []
    for k in rr.NAMES:
        if k not in base:
            continue
        for i in range(base[k].size):
            pair = []
            for sgn in (1.0, -1.0):
                d = {kk: v.copy() for kk, v in base.items()}
                d[k].reshape(-1)[i] += sgn * steps[k]
                pair.append(d)
            out.append((k, pair))
    return out


@pytest.mark.parametrize("shape", ["pnp10", "pnpl5+5"])
@pytest.mark.parametrize("loss", rc.ROBUST)
def test_finite_differences_of_the_references_minimiser(shape, loss):
    c = rc.case(f"{shape}-{loss}")
    b = 0
    out = host(c)
    assert out["vjp_status"][b] == 0
    args = ref_args(c, b)
    fd = []
    for k, (plus, minus) in _perturbations(c, b, STEPS):
        lp = rr.minimiser_value(*args[:5], args[5], args[6], **plus)
        lm = rr.minimiser_value(*args[:5], args[5], args[6], **minus)
        fd.append((lp - lm) / (2 * STEPS[k]))
    err = rr.rel_err(rr.flat(out, b), np.array(fd))
    print(f"{shape}-{loss}: {len(fd)} inputs, central differences of the reference's minimiser differ by {err:.2e} (relative L2)")
    assert err < FD_BAR


E2E_STEPS = {"pts_2d": 1e-3, "line_2d": 1e-3, "pts_3d": 1e-5, "line_3d": 1e-5, "weights_pts": 1e-3, "weights_lines": 1e-3}


@pytest.mark.parametrize("shape", ["pnp10", "pnpl5+5"])
@pytest.mark.parametrize("loss", rc.ROBUST)
def test_end_to_end_central_differences_through_the_forward(shape, loss):
    c = rc.case(f"{shape}-{loss}")
    b = 0
    K = rc.K_of(c["K"], b)
    GR, gt = c["GR"][b], c["gt"][b]
    fwd = dict(K=K, loss=loss, scale_px=c["delta"])
    base_kw = {k: v[None] for k, v in rc.one(c, b).items()}
    base = refine_pose_batch_robust_host(c["R"][b:b + 1], c["t"][b:b + 1], **base_kw, **fwd)
    assert base.status[0] == 0
    out = refine_vjp_robust_host(base.R, base.t, base.status, GR[None], gt[None], **base_kw, **fwd)
    assert out["vjp_status"][0] == 0
    pert = _perturbations(c, b, E2E_STEPS)
    batch = [d for _, pair in pert for d in pair]                        # every perturbed problem in ONE batch
    stack = {k: np.ascontiguousarray(np.stack([d[k] for d in batch])) for k in batch[0]}
    n = len(batch)
    res = refine_pose_batch_robust_host(np.repeat(base.R, n, 0), np.repeat(base.t, n, 0), **stack, **fwd)
    assert (res.status <= 1).all(), res.status     # (at the default 30 iterations a perturbed problem may stop at max_iters: its pose counts as it is)
    L = (res.R * GR).sum((1, 2)) + (res.t * gt).sum(1)
    fd = np.array([(L[2 * j] - L[2 * j + 1]) / (2 * E2E_STEPS[k]) for j, (k, _) in enumerate(pert)])
    err = rr.rel_err(rr.flat(out, 0), fd)
    print(f"{shape}-{loss}: {len(fd)} inputs, central differences through the forward differ by {err:.2e} (relative L2), "
          f"stationarity of the forward's pose {out['info'][0, 0]:.1e}")
    assert err < E2E_BAR


# ---- reductions -----------------------------------------------------------------------------------------------------------------------

def _ls(c, **kw):
    args = dict(K=c["K"], **c["kw"])
    args.update(kw)
    return refine_vjp_host(c["R"], c["t"], None, c["GR"], c["gt"], **args)


@pytest.mark.parametrize("name", ["pnp10-s1", "pnpl5+5-s1", "pnl6-s1"])
def test_l2_without_weights_is_the_least_squares_vjp(name):
    c = gc.case(name)
    want = _ls(c)
    got = refine_vjp_robust_host(c["R"], c["t"], None, c["GR"], c["gt"], K=c["K"], loss="l2", **c["kw"])
    assert (got["vjp_status"] == want["vjp_status"]).all()
    for k in CORR:
        if want[k] is not None:
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    # huber at a scale no residual reaches is l2, byte for byte
    hub = refine_vjp_robust_host(c["R"], c["t"], None, c["GR"], c["gt"], K=c["K"], loss="huber", scale_px=1e4, **c["kw"])
    for k in rr.NAMES:
        if got[k] is not None:
            assert hub[k].tobytes() == got[k].tobytes(), k
    assert hub["info"].tobytes() == got["info"].tobytes()


def test_weights_zero_and_one_are_a_mask():
    c, masks, _ = gc.masked_case()
    want = _ls(c, **masks)
    w = {"weights_pts": masks["mask_pts"].astype(np.float64), "weights_lines": masks["mask_lines"].astype(np.float64)}
    got = refine_vjp_robust_host(c["R"], c["t"], None, c["GR"], c["gt"], K=c["K"], loss="l2", **c["kw"], **w)
    assert (got["vjp_status"] == 0).all() and (want["vjp_status"] == 0).all()
    for k in CORR:
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    for k, m in (("weights_pts", "mask_pts"), ("weights_lines", "mask_lines")):
        assert not np.any(got[k][masks[m] == 0]) and np.all(got[k][masks[m] != 0] != 0.0), k


@pytest.mark.parametrize("name", ["pnpl5+5-huber", "pnpl5+5-cauchy", "contaminated-cauchy"])
def test_doubling_the_weights_halves_their_gradients_and_leaves_the_others(name):
    c = rc.case(name)
    ones = {k: (None if v is None else np.ones(v.shape[:2])) for k, v in (("weights_pts", c["kw"]["pts_3d"]), ("weights_lines", c["kw"]["line_3d"]))}
    w1 = {k: (ones[k] if c["w"][k] is None else c["w"][k]) for k in ones}
    w2 = {k: (None if v is None else 2.0 * v) for k, v in w1.items()}
    a, b = host(c, **w1), host(c, **w2)
    assert (a["vjp_status"] == 0).all() and (b["vjp_status"] == 0).all()
    for k in CORR:
        if a[k] is not None:
            assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(a[k]).max(), k
    for k in WGT:
        if a[k] is not None:
            assert np.abs(0.5 * a[k] - b[k]).max() <= 1e-12 * np.abs(a[k]).max(), k
    if all(v is None for v in c["w"].values()):   # absent weights are weights of 1
        z = host(c)
        for k in rr.NAMES:
            assert z[k].tobytes() == a[k].tobytes(), k


@pytest.mark.parametrize("loss", rc.ROBUST)
def test_weight_zero_over_spoiled_records_is_the_compacted_problem(loss):
    c, masks, live = gc.masked_case()
    rs = np.random.RandomState(8)
    n_p, n_l = masks["mask_pts"].shape[1], masks["mask_lines"].shape[1]
    B = len(c["R"])
    w = {"weights_pts": rs.uniform(0.25, 4.0, (B, n_p)) * masks["mask_pts"], "weights_lines": rs.uniform(0.25, 4.0, (B, n_l)) * masks["mask_lines"]}
    wl = {"weights_pts": np.ascontiguousarray(w["weights_pts"][:, masks["mask_pts"][0] != 0]),
          "weights_lines": np.ascontiguousarray(w["weights_lines"][:, masks["mask_lines"][0] != 0])}
    opts = dict(K=c["K"], loss=loss, scale_px=1.0)
    want = refine_vjp_robust_host(c["R"], c["t"], None, c["GR"], c["gt"], **live, **wl, **opts)
    got = refine_vjp_robust_host(c["R"], c["t"], None, c["GR"], c["gt"], **gc.spoiled(c["kw"], masks), **w, **opts)   # NaN / 1e9 behind w = 0
    assert want["vjp_status"].tolist() == got["vjp_status"].tolist()
    assert want["info"].tobytes() == got["info"].tobytes()
    for k in rr.NAMES:
        m = masks["mask_pts" if "pts" in k else "mask_lines"]
        off = m == 0
        assert off.any() and not np.any(got[k][off]) and not np.isnan(got[k]).any(), k              # exact zeros, weights' gradients too
        assert np.ascontiguousarray(got[k][~off]).reshape(want[k].shape).tobytes() == want[k].tobytes(), k


def test_a_bad_weight_is_status_3_unless_its_mask_hides_it():
    c = rc.case("pnpl5+5-huber")
    B = len(c["R"])
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        w = {k: v.copy() for k, v in c["w"].items()}
        w["weights_pts"][0, 2] = bad
        w["weights_lines"][1, 4] = bad
        out = host(c, **w)
        assert out["vjp_status"].tolist() == [3, 3], (bad, out["vjp_status"])
        assert all_zero(out) and np.isnan(out["info"]).all()
        mp, ml = np.ones((B, 5), np.uint8), np.ones((B, 5), np.uint8)
        mp[0, 2] = ml[1, 4] = 0
        hidden = host(c, mask_pts=mp, mask_lines=ml, **w)
        assert hidden["vjp_status"].tolist() == [0, 0], (bad, hidden["vjp_status"])
        assert not np.any(hidden["weights_pts"][0, 2]) and not np.any(hidden["weights_lines"][1, 4]) and not all_zero(hidden, 0)
    # the order of the checks: a bad weight before the count of live records, a skipped problem before both
    w = {k: v.copy() for k, v in c["w"].items()}
    w["weights_pts"][:, 0] = -2.0
    mp, ml = np.zeros((B, 5), np.uint8), np.zeros((B, 5), np.uint8)
    mp[:, 0] = 1
    assert host(c, mask_pts=mp, mask_lines=ml, **w)["vjp_status"].tolist() == [3, 3]
    assert host(c, mask_pts=mp, mask_lines=ml)["vjp_status"].tolist() == [2, 2]
    assert host(c, mask_pts=mp, mask_lines=ml, status=np.array([1, 0], np.int32), **w)["vjp_status"].tolist() == [1, 3]


def test_a_saddle_of_the_robust_cost_is_refused():
    s = rc.saddle()
    out = host(s)
    assert out["vjp_status"].tolist() == [2] and all_zero(out) and out["info"][0, 0] < 1e-10, out["info"]


def test_want_subsets_and_gradients_at_weights_of_one():
    c = rc.case("contaminated-huber")   # no weights: their gradients are the derivative at w = 1
    full = host(c)
    assert full["weights_pts"].shape == (3, 20) and full["weights_lines"].shape == (3, 10) and np.all(full["weights_pts"] != 0.0)
    only = host(c, want=("weights_lines",))
    assert [k for k in rr.NAMES if only[k] is not None] == ["weights_lines"]
    assert only["weights_lines"].tobytes() == full["weights_lines"].tobytes()
    with pytest.raises(ValueError, match="want"):
        host(c, want=("weights",))
    # the displaced records are the ones whose confidences matter least to the pose: their weights' gradients are the small ones
    d = c["displaced"]
    g = np.abs(np.concatenate([full["weights_pts"], full["weights_lines"]], 1))
    print("mean |dL/dw| displaced / clean:", g[d].mean() / g[~d].mean())
