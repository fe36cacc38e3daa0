"""The parts of the Levenberg-Marquardt schedule that the easy starts of tests/test_refine_host.py never reach, on the host path
(cvxpnpl_refine_batch_host) against the independent reference (tests/refine_reference.py): rejected trials and trials behind the camera,
lambda running out, max_iters of 0 to 3, a batch of unlike problems, scenes far from the world origin, and outputs that alias the inputs.
No GPU needed.

Measured (host, CPU): hard starts -- cost within 5e-14 of the reference's, poses within 1.4e-9, the reference's next step <= 1.1e-9; far
scenes at 1e2 / 1e4 / 1e6 -- poses within 1.2e-9 (R) and 1.8e-9 (t) of the unshifted run, cost within 3.8e-12 / 1.4e-9 / 6.3e-8, the
reference's next step with the scaled h <= 4e-11 / 3e-11 / 9e-10, covariance at 1e2 0.010 of its bound."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as rc
import refine_reference as ref


@pytest.fixture(scope="module")
def rf():
    from cvxpnpl_amd import build, refine

    build.build_refine()
    return refine


@pytest.mark.parametrize("shape", rc.HARD_SHAPES)
def test_hard_starts_reach_the_reference_s_minimum(rf, shape):
    """Starts 1.5 rad and 50 % of t off: the reference rejects trials on 2, 3 and 2 problems of the three shapes and meets a record behind
    the camera on one (asserted by the builder).  Trial counts are not compared: the library damps diag(J^T J) of its centred chart, the
    reference that of the public one, so after a single trial the two costs legitimately differ by tens of percent."""
    d, R0, t0, kw, runs = rc.hard_starts(shape)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, **kw)
    assert out.status.tolist() == [r["status"] for r in runs]
    cost = max(abs(r["cost"][1] - out.cost[b, 1]) / r["cost"][1] for b, r in enumerate(runs))
    pose = max(max(np.abs(r["R"] - out.R[b]).max(), np.abs(r["t"] - out.t[b]).max()) for b, r in enumerate(runs))
    nxt = rc.worst_next_step(d["K"], out.R, out.t, kw)
    print(f"{shape}: cost within {cost:.1e}, poses within {pose:.1e}, reference's next step <= {nxt:.1e}, trials <= {out.iters.max()}")
    assert cost <= 1e-9 and pose <= rc.STEP_BAR and nxt <= rc.STEP_BAR
    assert (out.cost[:, 1] <= out.cost[:, 0]).all()


@pytest.mark.parametrize("max_iters", [0, 1, 2, 3])
def test_small_max_iters(rf, max_iters):
    d, R0, t0, kw, runs = rc.hard_starts((10, 0))
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=max_iters, want_cov=True, **kw)
    assert (out.status == 1).all() and (out.iters == max_iters).all(), (out.status, out.iters)
    assert (out.cost[:, 1] <= out.cost[:, 0]).all()
    c0 = np.array([r["cost"][0] for r in runs])
    assert (np.abs(out.cost[:, 0] - c0) <= 1e-9 * c0).all()
    assert np.isfinite(out.R).all() and np.isfinite(out.t).all()
    if max_iters == 0:
        assert out.R.tobytes() == R0.tobytes() and out.t.tobytes() == t0.tobytes()                # bit for bit
        assert out.cost[:, 0].tobytes() == out.cost[:, 1].tobytes() and np.isfinite(out.cov).all()


def test_mixed_batch(rf):
    K, R0, t0, kw, expect = rc.mixed_batch()
    out = rf.refine_pose_batch_host(R0, t0, K=K, max_iters=100, want_cov=True, **kw)
    rc.check_mixed(out, R0, t0, expect)
    print(f"mixed batch: statuses {out.status.tolist()}, trials {out.iters.tolist()}")
    assert out.iters[rc.MIXED["collinear"][0]] >= 40                                            # the slow neighbour is slow
    live = rc.MIXED["ordinary"] + rc.MIXED["refined"] + rc.MIXED["hard"]
    assert rc.worst_next_step(K, out.R, out.t, kw, rows=live) <= rc.STEP_BAR
    for name in ("nan_pose", "behind", "nan_2d", "inf_3d", "nan_3d"):                           # the reference restates the contract
        b = rc.MIXED[name][0]
        r = ref.refine(K, R0[b], t0[b], max_iters=100, **rc.one(kw, b))
        assert r["status"] == out.status[b] and r["iters"] == 0 and r["R"].tobytes() == R0[b].tobytes(), name


@pytest.fixture(scope="module")
def unshifted(rf):
    d, R0, t0, kw, _ = rc.far_scene(0.0)
    return rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, **kw)


@pytest.mark.parametrize("offset", rc.FAR_OFFSETS)
def test_far_scenes_are_the_same_problem(rf, unshifted, offset):
    """The scene-centred chart exists for scenes far from the world origin.  (The reference differentiates in the public chart with
    h = ref.far_h: with its fixed 1e-3 it is the reference that fails here, not the library.)"""
    d, R0, t0, kw, o = rc.far_scene(offset)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, **kw)
    rc.check_far(out, unshifted, d, kw, o, offset)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def test_outputs_may_alias_the_inputs(rf):
    """include/cvxpnpl_amd_refine.h: R_out / t_out may alias the inputs.  The edge batch through the C entry itself, once into fresh
    arrays and once in place: every output byte for byte the same."""
    from cvxpnpl_amd import _lib

    K, R0, t0, kw, status_in, masks, expect = rc.edge_batch()
    L = _lib.refine_lib()
    o = rf._opts(100, 1e-10, 0.0)
    B = len(R0)

    def call(alias):
        R, t = R0.copy(), t0.copy()
        oR, ot = (R, t) if alias else (np.empty_like(R), np.empty_like(t))
        cost, cov = np.empty((B, 2)), np.empty((B, 6, 6))
        iters, st, n_live = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
        rcode = L.cvxpnpl_refine_batch_host(B, 8, _p(kw["pts_2d"]), _p(kw["pts_3d"]), 4, _p(kw["line_2d"]), _p(kw["line_3d"]), _p(K), 0, _p(R), _p(t),
                                            _p(status_in), 1, rf.ADMIT_USABLE, _p(masks["mask_pts"]), _p(masks["mask_lines"]), C.byref(o), _p(oR), _p(ot),
                                            _p(cost), _p(iters), _p(st), _p(n_live), _p(cov), 2)
        assert rcode == 0
        return rf.RefineResult(oR, ot, cost, iters, st, n_live, cov)

    a, b = call(False), call(True)
    rc.check_edge_batch(b, R0, t0, expect)
    for name, x, y in zip(a._fields, a, b):
        assert x.tobytes() == y.tobytes(), name
