"""The pose VJP (cvxpnpl_pose_vjp_host, the same source as the kernels) against finite differences -- no GPU.

Truth: the test's own local solver.  It takes the oracle's certified pose and polishes it by Gauss-Newton on (omega, tau) until the
stationarity residual |g| is at rounding level; only g = 0 matters here, so the check does not depend on the product's Hessian.
Central differences of the polished map theta -> (R, t), contracted with random (G_R, g_t), must match the VJP to 1e-6 relative.

Sensitivity (checked once by hand): with a Gauss-Newton H (the second-order term of the exponential left out of vjp_core.h's
solve_v), every case below misses this tolerance by orders of magnitude -- relative errors of 1e-3 ... 5e-2.
"""
import numpy as np
import pytest
from grad_reference import polish  # the test's own local solver (shared with test_pose_grad_reference.py)

from cvxpnpl_amd import synth
from cvxpnpl_amd.grad import ADMIT_CERTIFIED, ADMIT_RANK1, pose_vjp_host

K_GENERAL = np.array([[510.0, 2.5, 301.0], [0.0, 540.0, 262.0], [0.0, 0.0, 1.0]])


def _case(kind, n, seed, K=synth.K_KINECT, far=None):
    n_p, n_l = {"pnp": (n, 0), "pnl": (0, n), "pnpl": (n, n)}[kind]
    d = synth.make_pnpl(24, n_p, n_l, sigma=2.0, seed=seed, K=K)
    if far is not None:  # the same images, the world origin moved far from the scene
        d["pts_3d"] = d["pts_3d"] + far
        d["line_3d"] = d["line_3d"] + far
    return d, n_p, n_l


def _certified(orc, d, n_p, n_l):
    o = orc.pnpl_batch(d["pts_2d"] if n_p else None, d["line_2d"] if n_l else None, d["pts_3d"] if n_p else None,
                       d["line_3d"] if n_l else None, d["K"], eps=1e-11, max_iters=400000)
    # certified: the reference's absolute test (status 0), or -- for the larger noisy problems, whose cost is too big for an absolute
    # 1e-11 -- a rank-1 solution (status bit 2 only) whose SDP lower bound meets the primal objective to 1e-7 relative
    gap = np.abs(o["cost"][:, 0] - o["cost"][:, 1]) <= 1e-7 * np.abs(o["cost"][:, 0])
    return [b for b in range(len(o["status"])) if o["n_poses"][b] == 1 and (o["status"][b] == 0 or (o["status"][b] == 4 and gap[b]))], o


def _problem(d, b, n_p, n_l):
    e2 = lambda s: np.zeros(s)  # noqa: E731
    p2 = d["pts_2d"][b] if n_p else e2((0, 2))
    p3 = d["pts_3d"][b] if n_p else e2((0, 3))
    l2 = d["line_2d"][b] if n_l else e2((0, 2, 2))
    l3 = d["line_3d"][b] if n_l else e2((0, 2, 3))
    return p2, p3, l2, l3


def _vjp_one(R, t, p2, p3, l2, l3, K, GR, gt, status=0, admit=ADMIT_CERTIFIED):
    n_p, n_l = len(p3), len(l3)
    return pose_vjp_host(R[None], t[None], np.array([status], np.int32), GR[None], gt[None],
                         pts_2d=p2[None] if n_p else None, line_2d=l2[None] if n_l else None,
                         pts_3d=p3[None] if n_p else None, line_3d=l3[None] if n_l else None, K=K, admit_mask=admit, n_threads=1)


def _fd_check(R0, t0, p2, p3, l2, l3, K, rng):
    R, t, _ = polish(R0, t0, p2, p3, l2, l3, K)
    GR, gt = rng.standard_normal((3, 3)), rng.standard_normal(3)
    out = _vjp_one(R, t, p2, p3, l2, l3, K, GR, gt)
    assert out["vjp_status"][0] == 0
    scale3 = 1.0 + np.abs(np.concatenate([p3.ravel(), l3.ravel()])).max()
    worst = 0.0
    for name, arr, h in (("pts_2d", p2, 1e-3), ("pts_3d", p3, 1e-6 * scale3), ("line_2d", l2, 1e-3), ("line_3d", l3, 1e-6 * scale3)):
        if arr.size == 0:
            continue
        fd = np.zeros(arr.size)
        for k in range(arr.size):
            vals = []
            for sgn in (1.0, -1.0):
                a = arr.copy().ravel()
                a[k] += sgn * h
                a = a.reshape(arr.shape)
                args = {"pts_2d": (a, p3, l2, l3), "pts_3d": (p2, a, l2, l3), "line_2d": (p2, p3, a, l3), "line_3d": (p2, p3, l2, a)}[name]
                Rk, tk, _ = polish(R, t, *args, K)
                vals.append((GR * Rk).sum() + gt @ tk)
            fd[k] = (vals[0] - vals[1]) / (2 * h)
        got = out[name][0].ravel()
        rel = np.linalg.norm(got - fd) / np.linalg.norm(fd)
        worst = max(worst, rel)
        assert rel < 1e-6, (name, rel, got[:6], fd[:6])
    return worst


CASES = [("pnp", 4, 11, None, None), ("pnp", 6, 12, None, None), ("pnp", 10, 13, None, None), ("pnp", 50, 14, None, None),
         ("pnl", 6, 15, None, None), ("pnl", 10, 16, None, None), ("pnpl", 5, 17, None, None),
         ("pnp", 10, 18, K_GENERAL, None), ("pnpl", 5, 19, K_GENERAL, None),
         ("pnp", 10, 20, None, np.array([40.0, -25.0, 60.0])), ("pnpl", 5, 21, None, np.array([-30.0, 45.0, 20.0]))]


@pytest.mark.parametrize("kind,n,seed,K,far", CASES, ids=[f"{c[0]}{c[1]}{'-K' if c[3] is not None else ''}{'-far' if c[4] is not None else ''}"
                                                         for c in CASES])
def test_vjp_matches_finite_differences_of_the_polished_solve(orc, kind, n, seed, K, far):
    d, n_p, n_l = _case(kind, n, seed, **({"K": K} if K is not None else {}), far=far)
    ok, o = _certified(orc, d, n_p, n_l)
    assert len(ok) >= 2, o["status"]  # (at sigma = 2 px the reference's absolute gap test passes a fraction of the problems)
    rng = np.random.default_rng(seed)
    for b in ok[:2 if n >= 50 else 3]:
        _fd_check(o["R"][b, 0], o["t"][b, 0], *_problem(d, b, n_p, n_l), d["K"], rng)


def test_normal_component_of_G_R_gives_zero_gradient(orc):
    d, n_p, n_l = _case("pnpl", 5, 31)
    ok, o = _certified(orc, d, n_p, n_l)
    b = ok[0]
    R, t = o["R"][b, 0], o["t"][b, 0]
    S = np.random.default_rng(0).standard_normal((3, 3))
    out = _vjp_one(R, t, *_problem(d, b, n_p, n_l), d["K"], R @ (S + S.T), np.zeros(3))
    ref = _vjp_one(R, t, *_problem(d, b, n_p, n_l), d["K"], np.eye(3)[[1, 2, 0]], np.zeros(3))
    assert out["vjp_status"][0] == 0
    for name in ("pts_2d", "pts_3d", "line_2d", "line_3d"):
        assert np.abs(out[name]).max() < 1e-12 * np.abs(ref[name]).max(), name


def test_statuses_not_admitted_are_skipped_with_zero_gradients():
    d = synth.make_pnp(5, 8, sigma=1.0, seed=5)
    status = np.array([0, 1, 2, 3, 4], np.int32)
    rng = np.random.default_rng(1)
    kw = dict(pts_2d=d["pts_2d"], pts_3d=d["pts_3d"], K=d["K"])
    for admit, want in ((ADMIT_CERTIFIED, [0, 1, 1, 1, 1]), (ADMIT_RANK1, [0, 1, 0, 1, 0])):
        out = pose_vjp_host(d["R_gt"], d["t_gt"], status, rng.standard_normal((5, 3, 3)), rng.standard_normal((5, 3)), admit_mask=admit, **kw)
        assert list(out["vjp_status"]) == want
        for b in range(5):
            nz = np.abs(out["pts_2d"][b]).max() + np.abs(out["pts_3d"][b]).max()
            assert (nz > 0) == (want[b] == 0), (admit, b)
            if want[b] == 1:
                assert np.isnan(out["info"][b]).all()


def test_collinear_points_are_singular_with_zero_gradients():
    d = synth.make_pnp(1, 8, sigma=0.0, seed=6)
    s = np.linspace(-0.3, 0.3, 8)
    P = np.stack([s, 0.5 * s + 0.01, -0.2 * s], 1)[None]
    x = synth.project(P, d["K"], d["R_gt"], d["t_gt"])
    out = pose_vjp_host(d["R_gt"], d["t_gt"], np.zeros(1, np.int32), np.ones((1, 3, 3)), np.ones((1, 3)), pts_2d=x, pts_3d=P, K=d["K"])
    assert out["vjp_status"][0] == 2
    assert not out["pts_2d"].any() and not out["pts_3d"].any()


def test_nonfinite_pose_is_reported():
    d = synth.make_pnp(2, 8, sigma=1.0, seed=7)
    R = d["R_gt"].copy()
    R[1, 0, 0] = np.nan
    out = pose_vjp_host(R, d["t_gt"], np.zeros(2, np.int32), np.ones((2, 3, 3)), np.ones((2, 3)), pts_2d=d["pts_2d"], pts_3d=d["pts_3d"], K=d["K"])
    assert list(out["vjp_status"]) == [0, 3]
    assert not out["pts_2d"][1].any() and not out["pts_3d"][1].any()


def test_stationarity_of_certified_oracle_poses_is_reported(orc):
    for kind, n, seed in (("pnp", 10, 41), ("pnl", 10, 42), ("pnpl", 5, 43)):
        d, n_p, n_l = _case(kind, n, seed)
        ok, o = _certified(orc, d, n_p, n_l)
        for b in ok[:4]:
            out = _vjp_one(o["R"][b, 0], o["t"][b, 0], *_problem(d, b, n_p, n_l), d["K"], np.zeros((3, 3)), np.zeros(3))
            lo_hi, grel = out["info"][0]
            assert out["vjp_status"][0] == 0 and grel <= 1e-6, (kind, b, grel)
            assert 0 < lo_hi <= 1, lo_hi
            # and the polished pose is stationary to rounding
            _, _, g_pol = polish(o["R"][b, 0], o["t"][b, 0], *_problem(d, b, n_p, n_l), d["K"])
            assert g_pol < 1e-10


def test_rejects_bad_arguments():
    with pytest.raises(ValueError):
        pose_vjp_host(np.eye(3)[None], np.zeros((1, 3)), None, K=np.eye(3))
