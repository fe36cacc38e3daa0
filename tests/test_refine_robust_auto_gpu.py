"""The batch kernels of the twelfth library -- robust_scale_group_kernel<1 | 2 | 4 | 0>, refine_robust_pp_group_kernel<1 | 2 | 4 | 0> with
robust_w_pp_group_kernel, robust_cov_group_kernel -- against the host path of the same source and against the seventh library's device
call: every record count at which another kernel or another record of a lane comes into play, points, lines and both, batches that fill a
quarter of a wavefront, one and a quarter, and four and a quarter; masks, zero weights over spoiled records, and problems of status 2, 3
and 4 between good ones.

Bars (device against host, those of tests/test_refine_robust_gpu.py): statuses and counts equal; poses, sq and sigma 1e-8 (relative for sq
and sigma); the covariance within 100 of the reference's own floors of the host's, relative to |V|_F
(tests/test_refine_robust_auto_host.py), and within COV_DEVICE_HOST where the reference has not run.  Bit for bit: the device's med_sq
against numpy.median of the device's own live sq; a uniform scale array (on plain and on masked, zero-weighted and failing inputs), mixed
scales and the rounds against the calls they stand for."""
import ctypes as C

import numpy as np
import pytest
import torch

import refine_cases as rc
import refine_robust_auto_cases as ac
import refine_robust_auto_reference as ar

pytestmark = pytest.mark.gpu

COUNTS = (3, 4, 16, 17, 32, 33, 64, 65, 130)  # <1> | <1> full, <2> | <2> full, <4> | <4> full, <0> (re-reading) | <0> with nine records to a lane
KINDS = ("points", "lines", "mixed")
BATCHES = (1, 5, 17)                          # a quarter of a wavefront, one and a quarter, four and a quarter
STEP_TOL = 1e-7                               # (tests/test_refine_robust_gpu.py: the runs end by their step, host and device at the same trial)
COV_DEVICE_HOST = 1e-10                       # device against host covariance, of |V|_F, where no reference floor is at hand: the same sums in
                                              # another order (some 150 terms: 1e-14) through two solves with H, whose condition number in
                                              # these cases stays below 1e4.  Where the reference has run, the issue's bar holds: 100 floors.


@pytest.fixture(scope="module")
def ca():
    import cvxpnpl_amd

    return cvxpnpl_amd


def _split(n, kind):
    return {"points": (n, 0), "lines": (0, n), "mixed": (n - n // 3, n // 3)}[kind]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _np(res):
    return type(res)(*[x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in res])


def _dev_kw(kw):
    return {k: _dev(v) for k, v in kw.items() if v is not None}


def _problem(B, n_p, n_l, seed, hard):
    """B problems with (hard, and 16 records or more) every fourth record masked and spoiled and every fifth at weight 0 and spoiled, and
    (hard, and B >= 5) problems 1-4 made into status 2 (not admitted), 4 (a bad weight), 3 (two live records), 4 (behind the camera)."""
    d, R0, t0, kw = rc.problem(B, n_p, n_l, 1.0, seed=seed)
    kw = {k: (None if v is None else v.copy()) for k, v in kw.items()}
    t0 = t0.copy()
    n = n_p + n_l
    w, m, status = np.ones((B, n)), np.ones((B, n), np.uint8), np.zeros(B, np.int32)
    if hard and n >= 16:
        m[:, 3::4] = 0
        w[:, 4::5] = 0.0
    if hard and B >= 5:
        status[1] = 1
        w[2, 0] = np.nan
        m[3, 2:] = 0
        m[3, :2], w[3, :2] = 1, 1.0
        t0[4] = -t0[4]
    off = (m == 0) | (w == 0.0)
    for key2, key3, sel in (("pts_2d", "pts_3d", off[:, :n_p]), ("line_2d", "line_3d", off[:, n_p:])):
        if kw[key2] is not None:
            kw[key2][sel] = np.nan
            kw[key3][sel] = 1e9
    extra = {"weights_pts": np.ascontiguousarray(w[:, :n_p]) if n_p else None, "weights_lines": np.ascontiguousarray(w[:, n_p:]) if n_l else None,
             "mask_pts": np.ascontiguousarray(m[:, :n_p]) if n_p else None, "mask_lines": np.ascontiguousarray(m[:, n_p:]) if n_l else None}
    kw = {k: v for k, v in dict(kw, **extra).items() if v is not None}
    return d["K"], R0, t0, kw, status


def _check_scale(dev, host, what):
    assert dev.status.tolist() == host.status.tolist() and dev.n_live.tolist() == host.n_live.tolist(), (what, dev.status, host.status)
    worst = 0.0
    for b in range(len(host.status)):
        sq = dev.sq[b]
        if host.status[b] != 0:
            assert np.isnan(sq).all() and np.isnan(dev.sigma_px[b]) and np.isnan(dev.med_sq[b]), (what, b)
            continue
        live = host.sq[b] >= 0.0
        assert ((sq == -1.0) == ~live).all() and (host.sq[b][~live] == -1.0).all(), (what, b)
        np.testing.assert_allclose(sq[live], host.sq[b][live], rtol=1e-8, atol=0.0)
        worst = max(worst, abs(dev.sigma_px[b] - host.sigma_px[b]) / host.sigma_px[b])
        assert dev.med_sq[b].tobytes() == np.float64(np.median(sq[live])).tobytes(), (what, b)      # bit for bit, of the device's own sq
        want = np.sqrt(dev.med_sq[b] / ar.CHI2_2_MEDIAN)
        assert abs(dev.sigma_px[b] - want) <= 4.0 * np.spacing(want), (what, b)
    assert worst <= 1e-8, (what, worst)
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_scale_equals_the_host_path_and_its_median_is_exact(ca, n, kind):
    n_p, n_l = _split(n, kind)
    turn = COUNTS.index(n) * 3 + KINDS.index(kind)
    B = BATCHES[turn % 3]
    K, R0, t0, kw, status = _problem(B, n_p, n_l, 300 + turn, hard=True)
    Kb = K if turn % 2 else np.stack([K * np.array([[1.0 + 0.002 * b], [1.0], [1.0]]) for b in range(B)])
    host = ca.robust_scale_batch_host(R0, t0, K=Kb, status=status, admit_mask=1, **kw)
    table = np.full((B, 4), 7, np.int32)
    table[:, 0] = status
    st_dev = _dev(table)[:, 0] if turn % 2 else _dev(status)                                       # a strided column, or a plain vector
    dev = _np(ca.robust_scale_batch(_dev(R0), _dev(t0), K=_dev(Kb), status=st_dev, admit_mask=1, **_dev_kw(kw)))
    if B >= 5:
        assert host.status[:5].tolist() == [0, 2, 4, 3, 4]
    worst = _check_scale(dev, host, (n, kind))
    if B >= 5:                                                                                    # the neighbours of the bad ones are unaffected
        alone = _np(ca.robust_scale_batch(_dev(R0[:1]), _dev(t0[:1]), K=_dev(Kb[:1] if Kb.ndim == 3 else Kb), **_dev_kw({k: v[:1] for k, v in kw.items()})))
        assert alone.sigma_px[0].tobytes() == dev.sigma_px[0].tobytes() and alone.sq[0].tobytes() == dev.sq[0].tobytes()
    print(f"n = {n} {kind} B = {B}: sigma within {worst:.1e} of the host's")


def _same(a, b, what, fields=("R", "t", "cost", "iters", "status", "n_live", "robust_w", "n_inlier")):
    for name in fields:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (what, name)


@pytest.mark.parametrize("n", (16, 33, 64, 65))
def test_loop_at_a_scale_per_problem_against_the_seventh_library(ca, n):
    """A uniform scale array and a float are the seventh library's device call bit for bit; mixed scales are five batch-1 calls of the
    seventh library at the scalar scale bit for bit; bad scale elements give status 4 to their problem only."""
    n_p, n_l = _split(n, "mixed")
    B = 5
    K, R0, t0, kw, _ = _problem(B, n_p, n_l, 400 + n, hard=False)
    dkw, dR, dt, dK = _dev_kw(kw), _dev(R0), _dev(t0), _dev(K)
    mixed = np.array([0.5, 1.0, 2.0, 4.0, 8.0])
    for loss in ("l2", "huber", "cauchy"):
        want = _np(ca.refine_pose_batch_robust(dR, dt, K=dK, loss=loss, scale_px=1.5, step_tol=STEP_TOL, **dkw))
        for scale in (_dev(np.full(B, 1.5)), 1.5):
            got = _np(ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss=loss, scale_px=scale, step_tol=STEP_TOL, **dkw))
            _same(got, want, (n, loss, "uniform"))
        got = _np(ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss=loss, scale_px=_dev(mixed), step_tol=STEP_TOL, **dkw))
        assert (got.status <= 1).all() and got.scale_px.tobytes() == mixed.tobytes()
        for b in range(B):
            one = _np(ca.refine_pose_batch_robust(dR[b:b + 1], dt[b:b + 1], K=dK, loss=loss, scale_px=float(mixed[b]), step_tol=STEP_TOL,
                                                  **{k: v[b:b + 1] for k, v in dkw.items()}))
            for name in ("R", "t", "cost", "iters", "status", "n_live", "robust_w", "n_inlier"):
                assert getattr(got, name)[b].tobytes() == getattr(one, name)[0].tobytes(), (n, loss, b, name)
        if loss != "l2":
            bad = np.array([1.5, 0.0, 1.5, np.nan, -np.inf])
            gb = _np(ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss=loss, scale_px=_dev(bad), step_tol=STEP_TOL, covariance=True, **dkw))
            assert gb.status[[1, 3, 4]].tolist() == [4, 4, 4] and (gb.status[[0, 2]] <= 1).all()
            for b in (0, 2):
                for name in ("R", "t", "cost", "iters", "robust_w", "n_inlier"):
                    assert getattr(gb, name)[b].tobytes() == getattr(want, name)[b].tobytes(), (n, loss, b, name)
                assert np.isfinite(gb.cov[b]).all()
            for b in (1, 3, 4):
                assert gb.R[b].tobytes() == R0[b].tobytes() and gb.t[b].tobytes() == t0[b].tobytes()
                assert np.isnan(gb.cost[b]).all() and np.isnan(gb.robust_w[b]).all() and np.isnan(gb.scale_px[b]) and np.isnan(gb.cov[b]).all()
                assert gb.iters[b] == 0 and gb.n_inlier[b] == 0


@pytest.mark.parametrize("n,kind", ((16, "points"), (33, "mixed"), (64, "lines"), (130, "mixed")))
def test_loop_on_masks_zero_weights_and_bad_problems_against_the_seventh_library(ca, n, kind):
    """The per-problem-scale loop on the HARD inputs -- every fourth record masked and spoiled, every fifth at weight 0, problems of status
    2, 4, 3 and 4 between good ones, a strided status column -- against the seventh library's device call, bit for bit in every output of
    every problem; then a bad scale element on two good problems, with masks: status 4 for them, the others bit for bit as before."""
    n_p, n_l = _split(n, kind)
    B = 17
    K, R0, t0, kw, status = _problem(B, n_p, n_l, 450 + n, hard=True)
    dkw, dR, dt, dK = _dev_kw(kw), _dev(R0), _dev(t0), _dev(K)
    table = np.full((B, 3), 7, np.int32)
    table[:, 0] = status
    dst = _dev(table)[:, 0]
    for loss in ("l2", "huber", "cauchy"):
        want = _np(ca.refine_pose_batch_robust(dR, dt, K=dK, loss=loss, scale_px=1.5, status=dst, admit_mask=1, step_tol=STEP_TOL, **dkw))
        assert want.status[:5].tolist() == [want.status[0], 2, 4, 3, 4] and (want.status[5:] <= 1).all() and want.status[0] <= 1
        got = _np(ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss=loss, scale_px=_dev(np.full(B, 1.5)), status=dst, admit_mask=1, step_tol=STEP_TOL, **dkw))
        _same(got, want, (n, kind, loss, "hard"))
        assert got.R[1:5].tobytes() == R0[1:5].tobytes() and got.t[1:5].tobytes() == t0[1:5].tobytes()
        if loss != "l2":
            scale = np.full(B, 1.5)
            scale[[0, 9]] = [np.nan, 0.0]
            gb = _np(ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss=loss, scale_px=_dev(scale), status=dst, admit_mask=1, step_tol=STEP_TOL, **dkw))
            expect = want.status.copy()
            expect[[0, 9]] = 4
            assert gb.status.tolist() == expect.tolist()
            keep = np.ones(B, bool)
            keep[[0, 9]] = False
            for name in ("R", "t", "cost", "iters", "n_live", "robust_w", "n_inlier"):
                assert getattr(gb, name)[keep].tobytes() == getattr(want, name)[keep].tobytes(), (n, kind, loss, name)
            assert gb.R[[0, 9]].tobytes() == R0[[0, 9]].tobytes() and np.isnan(gb.robust_w[[0, 9]]).all() and np.isnan(gb.cost[[0, 9]]).all()


def test_rounds_are_explicit_calls_and_the_covariance_is_the_functional_form(ca):
    B, n_p, n_l = 17, 20, 10
    K, R0, t0, kw, status = _problem(B, n_p, n_l, 500, hard=True)
    dkw, dR, dt, dK, dst = _dev_kw(kw), _dev(R0), _dev(t0), _dev(K), _dev(status)
    got = ca.refine_pose_batch_robust_auto(dR, dt, K=dK, loss="cauchy", scale_rounds=2, scale_factor=2.0, scale_floor_px=0.25, covariance=True, status=dst,
                                           admit_mask=1, step_tol=STEP_TOL, **dkw)
    R, t, iters = dR, dt, 0
    for _ in range(2):
        est = ca.robust_scale_batch(R, t, K=dK, status=dst, admit_mask=1, **dkw)
        scale = torch.clamp(2.0 * est.sigma_px, min=0.25)
        step = ca.refine_pose_batch_robust_auto(R, t, K=dK, loss="cauchy", scale_px=scale, status=dst, admit_mask=1, step_tol=STEP_TOL, **dkw)
        R, t, iters = step.R, step.t, iters + step.iters
    g, s = _np(got), _np(step)
    assert g.status[:5].tolist() == [s.status[0], 2, 4, 3, 4] and (g.status[5:] <= 1).all()
    ok = g.status <= 1
    assert g.R[ok].tobytes() == s.R[ok].tobytes() and g.t[ok].tobytes() == s.t[ok].tobytes() and g.cost[ok].tobytes() == s.cost[ok].tobytes()
    assert (g.iters[ok] == iters.cpu().numpy()[ok]).all() and g.scale_px[ok].tobytes() == scale.cpu().numpy()[ok].tobytes()
    assert g.sigma_px[ok].tobytes() == est.sigma_px.cpu().numpy()[ok].tobytes()
    assert g.R[~ok].tobytes() == R0[~ok].tobytes() and g.t[~ok].tobytes() == t0[~ok].tobytes()       # the input pose, bit for bit
    assert np.isnan(g.scale_px[~ok]).all() and np.isnan(g.cov[~ok]).all() and (g.iters[~ok] == 0).all()
    cov = _np(ca.robust_covariance_batch(got.R, got.t, K=dK, loss="cauchy", scale_px=got.scale_px, status=got.status, **dkw))
    assert cov.cov.tobytes() == g.cov.tobytes() and cov.status.tobytes() == g.cov_status.tobytes()
    assert (cov.status[ok] == 0).all() and (cov.status[~ok] == 2).all() and np.isfinite(g.cov[ok]).all()
    host = ca.robust_covariance_host(g.R, g.t, K=K, loss="cauchy", scale_px=np.where(ok, g.scale_px, 1.0), status=g.status, **kw)
    assert host.status.tolist() == cov.status.tolist()
    rel = max(np.linalg.norm(g.cov[b] - host.cov[b]) / np.linalg.norm(host.cov[b]) for b in np.flatnonzero(ok))
    print(f"covariance of the rounds' result: device within {rel:.1e} of the host's, relative to |V|_F")
    assert rel <= COV_DEVICE_HOST


@pytest.mark.parametrize("kind,n_p,n_l,loss", (("clean", 10, 0, "cauchy"), ("clean", 5, 5, "l2"), ("contaminated", 20, 10, "huber")))
def test_covariance_against_the_host_path_and_the_reference(ca, kind, n_p, n_l, loss):
    case, refs = ac.cov_case(kind, n_p, n_l, loss)
    kw = ac.pack_kwargs(case)
    B = len(refs)
    host = ca.robust_covariance_host(case["R0"], case["t0"], K=case["K"], loss=loss, scale_px=case["delta"], **kw)
    dev = _np(ca.robust_covariance_batch(_dev(case["R0"]), _dev(case["t0"]), K=_dev(case["K"]), loss=loss, scale_px=case["delta"], **_dev_kw(kw)))
    each = _np(ca.robust_covariance_batch(_dev(case["R0"]), _dev(case["t0"]), K=_dev(case["K"]), loss=loss, scale_px=_dev(np.full(B, case["delta"])), **_dev_kw(kw)))
    assert dev.cov.tobytes() == each.cov.tobytes() and dev.status.tolist() == host.status.tolist() == [0] * B
    for b, (V, floor, _, _) in enumerate(refs):
        nv = np.linalg.norm(V)
        eh, er = np.linalg.norm(dev.cov[b] - host.cov[b]) / nv, np.linalg.norm(dev.cov[b] - V) / nv
        print(f"{case['name']} problem {b}: reference floor {floor:.2e}; device against host {eh:.2e}, against the reference {er:.2e}")
        assert eh <= 100.0 * floor and er <= 100.0 * floor, (eh, er, floor)


def test_outputs_may_alias_the_input_pose(ca):
    from cvxpnpl_amd import _lib
    from cvxpnpl_amd.api import _ptr

    B, n_p = 17, 33
    K, R0, t0, kw, status = _problem(B, n_p, 0, 600, hard=True)
    dkw, dK = _dev_kw(kw), _dev(K)
    scale = _dev(np.linspace(0.5, 4.0, B))
    want = _np(ca.refine_pose_batch_robust_auto(_dev(R0), _dev(t0), K=dK, loss="huber", scale_px=scale, status=_dev(status), admit_mask=1, **dkw))
    R, t, st = _dev(R0), _dev(t0), _dev(status)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    cost, rw = torch.empty((B, 2), **f64), torch.empty((B, n_p), **f64)
    iters, ost, n_live, n_in = (torch.empty((B,), **i32) for _ in range(4))
    L = _lib.refine_robust_auto_lib()
    o = _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), 30, 1e-10, 1e-3, _lib.LOSS_HUBER, 1.0)
    rc_ = L.cvxpnpl_refine_robust_pp_batch(B, n_p, _ptr(dkw["pts_2d"]), _ptr(dkw["pts_3d"]), 0, None, None, _ptr(dK), 0, _ptr(R), _ptr(t), _ptr(st), 1, 1,
                                           _ptr(dkw["mask_pts"]), None, _ptr(dkw["weights_pts"]), None, _ptr(scale), C.byref(o), _ptr(R), _ptr(t), _ptr(cost),
                                           _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw), _ptr(n_in), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, L.cvxpnpl_refine_robust_auto_last_error()
    torch.cuda.synchronize()
    assert ost.cpu().numpy().tolist() == want.status.tolist()
    ok = want.status <= 1
    assert R.cpu().numpy()[ok].tobytes() == want.R[ok].tobytes() and t.cpu().numpy()[ok].tobytes() == want.t[ok].tobytes()
    assert R.cpu().numpy()[~ok].tobytes() == R0[~ok].tobytes() and t.cpu().numpy()[~ok].tobytes() == t0[~ok].tobytes()
    assert cost.cpu().numpy()[ok].tobytes() == want.cost[ok].tobytes() and rw.cpu().numpy()[ok].tobytes() == want.robust_w[ok].tobytes()
