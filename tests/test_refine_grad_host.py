"""The host path of the refinement's backward pass (cvxpnpl_refine_vjp_batch_host; csrc/refine_vjp_core.h, the source of the kernels)
against an independent float64 autograd reference (tests/refine_grad_reference.py: the residuals' definition, torch.matrix_exp, double
backward) at the reference's own polished poses (tests/refine_grad_cases.py) -- no GPU.

Error: relative L2 per problem over all four gradients.  Measured over the 16 cases (every problem of every case): worst
host-vs-reference error 8.5e-13 (pnl3-s0, a minimal line problem with a pivot ratio of 0.03; below 4e-14 for every other case away from
the far scenes), worst floor of the reference (centred against plain chart) 3.2e-12.  BOUND = 1e-10 is 100 x the worst error, rounded
up: the error grows with cond(H), which varies by orders across seeds.  The floor is asserted below BOUND.
The two scenes shifted 1e4 from the origin are held to BOUND_FAR = 2e-9, 100 x their measured 1.9e-11: there t is stored to
eps |t| = 2e-12, the library forms R c + t and the reference R X + t from it with roundings of that size, so the two differentiate poses
2e-12 apart.  The PLAIN chart of the reference loses |c|^2 = 1e8 there (measured floor 9.9e-7; this is why the library centres its
chart and why the centred reference is the truth); that floor is asserted below FLOOR_FAR = 1e-4 only.

Gauss-Newton: on every noisy over-determined case the host path's distance to the reference WITH the Gauss-Newton Hessian is at least
1e3 x its distance to the full one (measured: 4.5e7 x at the least, the Gauss-Newton gradients being off by 8e-4 .. 2e-2 relative).

End to end: central differences of <G_R, R> + <g_t, t> through refine_pose_batch_host (step_tol 1e-14, max_iters 100) over every input
coordinate, steps 1e-3 px and 1e-5 scene units.  Measured relative L2 error 5.2e-6 (10 points) and 1.0e-4 (5 + 5: the forward ends
at the rounding floor of its cost, poses good to 1e-8, over steps of 1e-5); the bar is 1e-2, a coarse one that a sign or chart error
(relative error of order 1) cannot pass, with a margin of 100 over the differences' own noise.
"""
import numpy as np
import pytest
import torch

import refine_grad_cases as gc
import refine_grad_reference as rg
from cvxpnpl_amd.refine import refine_pose_batch_host
from cvxpnpl_amd.refine_grad import pose_passthrough, refine_vjp_host

BOUND = 1e-10
BOUND_FAR = 2e-9
FLOOR_FAR = 1e-4
E2E_BAR = 1e-2


def host(c, **kw):
    args = dict(K=c["K"], **c["kw"])
    args.update(kw)
    return refine_vjp_host(c["R"], c["t"], args.pop("status", None), args.pop("grad_R", c["GR"]), args.pop("grad_t", c["gt"]), **args)


def all_zero(out, b=None):
    return all(not np.any(v if b is None else v[b]) for k, v in out.items() if k in rg.NAMES and v is not None)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_host_matches_the_autograd_reference(name):
    c = gc.case(name)
    out = host(c)
    far = gc.CASES[name][5].get("far", False)
    worst = worst_floor = 0.0
    for b in range(len(c["R"])):
        assert out["vjp_status"][b] == 0, (name, b, out["vjp_status"])
        truth, floor = rg.truth_and_floor(c["R"][b], c["t"][b], gc.K_of(c["K"], b), c["GR"][b], c["gt"][b], **gc.one(c["kw"], b))
        worst, worst_floor = max(worst, rg.rel_err(rg.flat(out, b), truth)), max(worst_floor, floor)
    print(f"{name}: worst host-vs-reference {worst:.2e}, worst floor (plain chart) {worst_floor:.2e}, info {out['info'].max(0)}")
    assert worst < (BOUND_FAR if far else BOUND), (name, worst)
    assert worst_floor < (FLOOR_FAR if far else BOUND), (name, worst_floor)


@pytest.mark.parametrize("name", gc.NOISY)
def test_the_hessian_is_the_full_one_not_gauss_newton(name):
    c = gc.case(name)
    out = host(c)
    for b in range(len(c["R"])):
        args = (c["R"][b], c["t"][b], gc.K_of(c["K"], b), c["GR"][b], c["gt"][b])
        full = rg.flat(rg.reference_vjp(*args, **gc.one(c["kw"], b)))
        gn = rg.flat(rg.reference_vjp(*args, hessian="gn", **gc.one(c["kw"], b)))
        got = rg.flat(out, b)
        d_full, d_gn = rg.rel_err(got, full), rg.rel_err(got, gn)
        print(f"{name}[{b}]: to the full reference {d_full:.2e}, to the Gauss-Newton one {d_gn:.2e}")
        assert d_gn >= 1e3 * d_full and d_gn > 1e-6, (name, b, d_full, d_gn)


@pytest.mark.parametrize("name", ["pnp10-s1", "pnpl5+5-s1"])
def test_end_to_end_central_differences_through_the_refinement(name):
    c = gc.case(name)
    b = 0
    K, kw = c["K"], {k: (None if v is None else v[b:b + 1]) for k, v in c["kw"].items()}
    GR, gt = c["GR"][b], c["gt"][b]
    fwd = dict(K=K, max_iters=100, step_tol=1e-14, status=None)
    base = refine_pose_batch_host(c["R"][b:b + 1], c["t"][b:b + 1], **kw, **fwd)
    assert base.status[0] == 0
    out = refine_vjp_host(base.R, base.t, base.status, GR[None], gt[None], K=K, **kw)
    assert out["vjp_status"][0] == 0
    keys = [k for k in rg.NAMES if kw[k] is not None]
    steps = {"pts_2d": 1e-3, "line_2d": 1e-3, "pts_3d": 1e-5, "line_3d": 1e-5}
    # every perturbed problem in ONE batch: 2 per input coordinate
    batch, where = [], []
    for k in keys:
        for i in range(kw[k][0].size):
            for sgn in (1.0, -1.0):
                d = {kk: (None if v is None else v[0].copy()) for kk, v in kw.items()}
                d[k].reshape(-1)[i] += sgn * steps[k]
                batch.append(d)
            where.append((k, i))
    stack = {k: (None if kw[k] is None else np.stack([d[k] for d in batch])) for k in kw}
    n = len(batch)
    res = refine_pose_batch_host(np.repeat(base.R, n, 0), np.repeat(base.t, n, 0), **stack, **fwd)
    assert (res.status == 0).all()
    L = (res.R * GR).sum((1, 2)) + (res.t * gt).sum(1)
    fd = np.array([(L[2 * j] - L[2 * j + 1]) / (2 * steps[k]) for j, (k, _) in enumerate(where)])
    err = rg.rel_err(rg.flat(out, 0), fd)
    print(f"{name}: {len(fd)} input coordinates, central differences through the refinement differ by {err:.2e} (relative L2)")
    assert err < E2E_BAR


def test_records_that_are_not_live_get_zero_and_change_nothing():
    c, masks, live = gc.masked_case()
    want = host(dict(c, kw=live))
    for kw in (c["kw"], gc.spoiled(c["kw"], masks)):          # NaN / 1e9 in the masked records change nothing
        out = host(dict(c, kw=kw), **masks)
        assert (out["vjp_status"] == 0).all() and (want["vjp_status"] == 0).all()
        for k2, k3, m in (("pts_2d", "pts_3d", "mask_pts"), ("line_2d", "line_3d", "mask_lines")):
            off = masks[m] == 0
            for k in (k2, k3):
                assert off.any() and not np.any(out[k][off]), k                  # exactly zero
                got = out[k][~off].reshape(want[k].shape)
                assert np.abs(got - want[k]).max() <= 1e-9 * np.abs(want[k]).max(), k
    # a line with a = b is not live either
    kw = {k: v.copy() for k, v in c["kw"].items()}
    dead = 1
    assert masks["mask_lines"][0, dead] == 1
    kw["line_2d"][:, dead, 1] = kw["line_2d"][:, dead, 0]
    out = host(dict(c, kw=kw), **masks)
    ml = masks["mask_lines"].copy()
    ml[:, dead] = 0
    ref = host(c, mask_pts=masks["mask_pts"], mask_lines=ml)
    assert not np.any(out["line_2d"][:, dead]) and not np.any(out["line_3d"][:, dead])
    for k in rg.NAMES:
        assert out[k].tobytes() == ref[k].tobytes(), k


def test_statuses_and_zero_gradients():
    c = gc.case("pnpl5+5-s1")
    B = len(c["R"])
    # not admitted
    out = host(c, status=np.array([0, 1, 3], np.int32))
    assert out["vjp_status"].tolist() == [0, 1, 1] and all_zero(out, 1) and all_zero(out, 2) and not all_zero(out, 0)
    out = host(c, status=np.array([0, 1, 3], np.int32), admit_mask=0x2)
    assert out["vjp_status"].tolist() == [1, 0, 1]
    # det R < 0, a NaN pose
    R = c["R"].copy()
    R[0, 1] = -R[0, 1]
    R[1, 2, 2] = np.nan
    out = host(dict(c, R=R))
    assert out["vjp_status"].tolist() == [1, 1, 0] and all_zero(out, 0) and all_zero(out, 1) and np.isnan(out["info"][:2]).all()
    # two live records
    mp, ml = np.zeros((B, 5), np.uint8), np.zeros((B, 5), np.uint8)
    mp[:, 0] = ml[:, 3] = 1
    out = host(c, mask_pts=mp, mask_lines=ml)
    assert (out["vjp_status"] == 2).all() and all_zero(out)
    # a stationary point that is not a minimum
    s = gc.saddle()
    out = host(s)
    assert out["vjp_status"].tolist() == [2] and all_zero(out) and out["info"][0, 0] < 1e-10, out["info"]
    # a record behind the camera, NaN in a live record
    t = c["t"].copy()
    Y = c["kw"]["pts_3d"][0, 2] @ c["R"][0].T
    t[0, 2] = -Y[2] - 0.1
    kw = {k: v.copy() for k, v in c["kw"].items()}
    kw["line_3d"][1, 4, 1, 0] = np.nan
    kw["pts_2d"][2, 0, 1] = np.inf
    out = host(dict(c, t=t, kw=kw))
    assert out["vjp_status"].tolist() == [3, 3, 3] and all_zero(out)
    # a non-finite upstream gradient
    GR = c["GR"].copy()
    GR[1, 0, 0] = np.nan
    out = host(dict(c, GR=GR))
    assert out["vjp_status"].tolist() == [0, 3, 0] and all_zero(out, 1)
    # missing upstream gradients count as zero
    a, z = host(c, grad_R=None), host(c, grad_R=np.zeros_like(c["GR"]))
    assert rg.flat(a).tobytes() == rg.flat(z).tobytes()
    assert all_zero(host(c, grad_R=None, grad_t=None)) and (host(c, grad_R=None, grad_t=None)["vjp_status"] == 0).all()
    # want subsets: the others absent
    out = host(c, want=("pts_3d",))
    assert out["pts_2d"] is None and out["line_2d"] is None and out["line_3d"] is None
    assert out["pts_3d"].tobytes() == host(c)["pts_3d"].tobytes()


def test_a_pose_stopped_short_shows_in_info():
    c = gc.case("pnp10-s1")
    K, kw = c["K"], c["kw"]
    rs = np.random.RandomState(3)
    R0 = np.stack([rg.pose_of(rg._t(0.3 * rs.normal(size=6) * np.array([1, 1, 1, 0, 0, 0])), rg._t(R), rg._t(t), rg._t(np.zeros(3)))[0].numpy()
                   for R, t in zip(c["R"], c["t"])])
    short = refine_pose_batch_host(R0, c["t"] * 1.2, K=K, max_iters=1, **kw)
    assert (short.status == 1).all()
    out = refine_vjp_host(short.R, short.t, short.status, c["GR"], c["gt"], K=K, admit_mask=0x3, **kw)
    full = host(c)
    print("stationarity of the poses stopped after one trial:", out["info"][:, 0], "of the polished ones:", full["info"][:, 0])
    assert (out["info"][:, 0] > 1e-6).all() and (full["info"][:, 0] < 1e-10).all()
    assert (refine_vjp_host(short.R, short.t, short.status, c["GR"], c["gt"], K=K, **kw)["vjp_status"] == 1).all()  # max_iters is not admitted by default


def test_pose_passthrough_rule():
    status = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)
    gR, gt = torch.randn(5, 3, 3, dtype=torch.float64), torch.randn(5, 3, dtype=torch.float64)
    pR, pt = pose_passthrough(status, gR, gt)
    assert not pR[:2].any() and not pt[:2].any()                                  # a minimiser does not depend on its start
    assert pR[2:].numpy().tobytes() == gR[2:].numpy().tobytes() and pt[2:].numpy().tobytes() == gt[2:].numpy().tobytes()
    assert pose_passthrough(status, None, gt)[0] is None and pose_passthrough(status, gR, None)[1] is None
    # the forward rule it mirrors: for status 2-4 the host refinement returns the input pose bit for bit
    c = gc.case("pnp10-s1")
    R = c["R"].copy()
    R[1, 0] = -R[1, 0]
    res = refine_pose_batch_host(R, c["t"], K=c["K"], status=np.array([0, 0, 1], np.int32), **c["kw"])
    assert res.status.tolist() == [0, 2, 2]
    assert res.R[1:].tobytes() == R[1:].tobytes() and res.t[1:].tobytes() == c["t"][1:].tobytes()
