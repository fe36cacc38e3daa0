"""refine_robust_group_kernel<1 | 2 | 4 | 0> and robust_w_group_kernel (the batch form of the robust refinement) against the host path of the
same source: every record count at which another kernel or another record of a lane comes into play, every loss, weights, zero weights
over spoiled records, partly filled wavefronts, a camera per problem, a strided status column; and the independence of the problems
of a batch.

Bars (device against host): statuses, n_live, n_inlier equal; poses 1e-8; costs 1e-9 relative; robust_w 1e-8.  The cost AFTER of a problem
with three live records (six residuals, six unknowns: the minimum is an exact fit) is a rounding residue of 1e-25 in which two runs share
no digit; there both are held below 1e-9 of the cost before.

The step tolerance of these comparisons is 1e-7, not the default 1e-10, and the trial counts are then asserted equal.  On a curved loss the
iteration converges linearly (the rho'' term is dropped), so at 1e-10 a run does not end by its step but by the schedule's rounding-floor
rule -- two costs that agree to 1e-12 -- at steps of some 5e-9, and whether that rule fires at trial n or n + 1 is decided by the rounding
of the two sums: the schedule's own header calls it chance.  Host and device sum in different orders.  Measured at the default tolerance on
the 187 comparisons of this file: 184 agree to 6e-15 in the pose and 1.3e-12 in robust_w; in 3 (17 lines cauchy, 33 lines huber with zero
weights, 7 + 3 huber) one side takes one more trial, the poses then differ by 1.4e-9 - 2.5e-9 (inside their bar) and robust_w, which
moves by |d rho' / d pose| ~ 200 per rad, by 2.8e-7 - 5.1e-7 (outside its bar).  That is a difference of one trial of a correct schedule,
not of the arithmetic under test; with the run ended by its step -- a comparison with a margin of 1e-10 relative, not 1e-4 -- both sides stop
at the same trial and every bar is held as the issue states it.  tests/test_refine_robust_scenes_gpu.py runs at the default tolerance."""
import numpy as np
import pytest
import torch

import refine_cases as rc
import refine_robust_cases as cases

pytestmark = pytest.mark.gpu

COUNTS = (3, 16, 17, 32, 33, 64, 65)          # <1> | <1> full, <2> | <2> full, <4> | <4> full, <0> (re-reading)
KINDS = ("points", "lines", "mixed")
BATCHES = (1, 3, 4, 5)                        # a quarter of a wavefront, three quarters, a full one, one and a quarter
DELTA = 1.5
STEP_TOL = 1e-7                               # (see above)


@pytest.fixture(scope="module")
def rb():
    from cvxpnpl_amd import refine_robust

    return refine_robust


def _split(n, kind):
    return {"points": (n, 0), "lines": (0, n), "mixed": (n - n // 3, n // 3)}[kind]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _np_result(res):
    return type(res)(*[x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in res])


def _weights(variant, B, n_p, n_l, kw, seed):
    """(weights_pts, weights_lines, kw): None / random in [0.1, 2] / random with every third record (counted through points then lines) at
    weight 0 and its data spoiled (NaN in the 2D half, 1e9 in the 3D half)."""
    if variant == "none":
        return None, None, kw
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.1, 2.0, (B, n_p + n_l))
    if variant == "zeros":
        w[:, 2::3] = 0.0
        masks = rc.boundary_masks(n_p, n_l, B)                 # the same every-third pattern, as masks: for spoil_masked only
        kw = rc.spoil_masked(kw, masks)
    return (np.ascontiguousarray(w[:, :n_p]) if n_p else None), (np.ascontiguousarray(w[:, n_p:]) if n_l else None), kw


def _compare(dev, host, R0, t0, what):
    assert dev.status.tolist() == host.status.tolist(), (what, dev.status, host.status)
    assert dev.n_live.tolist() == host.n_live.tolist() and dev.n_inlier.tolist() == host.n_inlier.tolist(), (what, dev.n_inlier, host.n_inlier)
    assert dev.iters.tolist() == host.iters.tolist(), (what, dev.iters, host.iters)
    done = host.status <= 1
    worst = {"pose": 0.0, "cost": 0.0, "w": 0.0}
    for b in range(len(R0)):
        if done[b]:
            worst["pose"] = max(worst["pose"], np.abs(dev.R[b] - host.R[b]).max(), np.abs(dev.t[b] - host.t[b]).max())
            rel = np.abs(dev.cost[b] - host.cost[b]) / np.abs(host.cost[b])
            if host.n_live[b] == 3:                                                          # an exact fit: see the head of the file
                assert dev.cost[b, 1] <= 1e-9 * host.cost[b, 0] and host.cost[b, 1] <= 1e-9 * host.cost[b, 0], (what, b, dev.cost[b], host.cost[b])
                rel = rel[:1]
            worst["cost"] = max(worst["cost"], rel.max())
            worst["w"] = max(worst["w"], np.abs(dev.robust_w[b] - host.robust_w[b]).max())
            assert dev.cost[b, 1] <= dev.cost[b, 0]
        else:
            assert dev.R[b].tobytes() == R0[b].tobytes() and dev.t[b].tobytes() == t0[b].tobytes(), (what, b)      # bit for bit
            assert np.isnan(dev.cost[b]).all() and dev.iters[b] == 0 and np.isnan(dev.robust_w[b]).all() and dev.n_inlier[b] == 0, (what, b)
    print(f"{what}: poses within {worst['pose']:.1e}, costs within {worst['cost']:.1e}, robust_w within {worst['w']:.1e}")
    assert worst["pose"] <= 1e-8 and worst["cost"] <= 1e-9 and worst["w"] <= 1e-8, (what, worst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_device_equals_host(rb, n, kind):
    """One record count and kind: the three losses x (no weights, random weights, every third record at weight 0 and spoiled), the batch
    size, the camera per problem and the strided status column taken in turn, so that each occurs with each kernel."""
    n_p, n_l = _split(n, kind)
    turn = COUNTS.index(n) * 3 + KINDS.index(kind)
    for i, (loss, variant) in enumerate((l, v) for l in ("l2", "huber", "cauchy") for v in ("none", "random", "zeros")):
        B = BATCHES[(turn + i) % 4]
        d, R0, t0, kw = rc.problem(B, n_p, n_l, 1.0, seed=100 + turn)
        wp, wl, kw = _weights(variant, B, n_p, n_l, kw, seed=turn)
        K = d["K"] if (turn + i) % 2 else np.stack([d["K"] * np.array([[1.0 + 0.002 * b], [1.0], [1.0]]) for b in range(B)])
        status = np.zeros(B, np.int32)
        if B > 1:
            status[B - 1] = 1                                                            # not admitted: passes through
        table = np.full((B, 4), 7, np.int32)
        table[:, 0] = status
        st_dev = _dev(table)[:, 0] if i % 3 == 0 else _dev(status)                          # a strided column, or a plain vector
        host = rb.refine_pose_batch_robust_host(R0, t0, K=K, loss=loss, scale_px=DELTA, weights_pts=wp, weights_lines=wl, status=status, max_iters=100,
                                                step_tol=STEP_TOL, **kw)
        dev = rb.refine_pose_batch_robust(_dev(R0), _dev(t0), K=_dev(K), loss=loss, scale_px=DELTA, weights_pts=_dev(wp), weights_lines=_dev(wl),
                                          status=st_dev, max_iters=100, step_tol=STEP_TOL, **{k: _dev(v) for k, v in kw.items()})
        _compare(_np_result(dev), host, R0, t0, f"{n_p}+{n_l} {loss} {variant} B={B}")
        if variant == "zeros":
            assert (host.n_live[: max(B - 1, 1)] == n - len(range(2, n, 3))).all()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", [10, 20, 40, 70])
def test_every_kernel_at_every_batch_size(rb, n, B):
    n_p, n_l = _split(n, "mixed")
    d, R0, t0, kw = rc.problem(B, n_p, n_l, 1.0, seed=7 * n + B)
    host = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], loss="huber", scale_px=DELTA, max_iters=100, step_tol=STEP_TOL, **kw)
    dev = rb.refine_pose_batch_robust(_dev(R0), _dev(t0), K=_dev(d["K"]), loss="huber", scale_px=DELTA, max_iters=100, step_tol=STEP_TOL,
                                      **{k: _dev(v) for k, v in kw.items()})
    assert (host.status == 0).all()
    _compare(_np_result(dev), host, R0, t0, f"{n_p}+{n_l} B={B}")


def test_outputs_may_alias_the_input_pose(rb):
    d, R0, t0, kw = rc.problem(5, 12, 6, 1.0, seed=3)
    dk = {k: _dev(v) for k, v in kw.items()}
    want = _np_result(rb.refine_pose_batch_robust(_dev(R0), _dev(t0), K=_dev(d["K"]), loss="cauchy", scale_px=DELTA, max_iters=100, **dk))
    from cvxpnpl_amd import _lib
    from cvxpnpl_amd.api import _ptr
    import ctypes as C

    R, t = _dev(R0), _dev(t0)
    cost, rw = torch.empty((5, 2), dtype=torch.float64, device="cuda"), torch.empty((5, 18), dtype=torch.float64, device="cuda")
    iters, st, n_live, n_in = (torch.empty(5, dtype=torch.int32, device="cuda") for _ in range(4))
    o = _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), 100, 1e-10, 1e-3, _lib.LOSS_CAUCHY, DELTA)
    Kd = _dev(d["K"])
    rc_ = _lib.refine_robust_lib().cvxpnpl_refine_robust_batch(
        5, 12, _ptr(dk["pts_2d"]), _ptr(dk["pts_3d"]), 6, _ptr(dk["line_2d"]), _ptr(dk["line_3d"]), _ptr(Kd), 0, _ptr(R), _ptr(t), None, 1, 0x5, None, None,
        None, None, C.byref(o), _ptr(R), _ptr(t), _ptr(cost), _ptr(iters), _ptr(st), _ptr(n_live), _ptr(rw), _ptr(n_in),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0
    assert R.cpu().numpy().tobytes() == want.R.tobytes() and t.cpu().numpy().tobytes() == want.t.tobytes()
    assert cost.cpu().numpy().tobytes() == want.cost.tobytes() and rw.cpu().numpy().tobytes() == want.robust_w.tobytes()
    assert n_in.cpu().tolist() == want.n_inlier.tolist()


# ---- independence of the problems of a batch -------------------------------------------------------------------------------------------

ROWS = {"contaminated": (0, 4, 8), "one_trial": (1,), "not_admitted": (2,), "nan_pose": (3,), "three_live": (5,), "two_live": (6,), "behind": (7,),
        "negative_weight": (9,), "clean": (10,), "reflection": (11,)}
UNLIKE_MAX_ITERS = 7


def _unlike(rb):
    """Twelve unlike problems of 20 points + 10 lines under the Cauchy loss at delta = 2, ordered so that each wavefront of four holds
    unlike neighbours: case (b) three times, a start at the minimum (one trial), every pass-through status, a negative weight, fewer
    than three live records through zero weights, and a run cut off by max_iters."""
    case = cases.contaminated("cauchy")
    d, Rc, tc, kwc = rc.problem(12, 20, 10, 0.5, seed=71)
    kw = {k: v.copy() for k, v in kwc.items()}
    R0, t0 = Rc.copy(), tc.copy()
    wp, wl = np.ones((12, 20)), np.ones((12, 10))
    status = np.zeros(12, np.int32)
    for row, b in zip(ROWS["contaminated"], range(3)):
        for k in kw:
            kw[k][row] = case["kw"][k][b]
        R0[row], t0[row] = case["R0"][b], case["t0"][b]
    row = ROWS["one_trial"][0]                                   # the host's own minimum of the clean problem in this row
    h = rb.refine_pose_batch_robust_host(R0[row:row + 1], t0[row:row + 1], K=d["K"], loss="cauchy", scale_px=2.0, max_iters=100,
                                         **{k: v[row:row + 1] for k, v in kw.items()})
    assert h.status[0] == 0
    R0[row], t0[row] = h.R[0], h.t[0]
    status[ROWS["not_admitted"][0]] = 1
    R0[ROWS["nan_pose"][0], 2, 1] = np.nan
    R0[ROWS["reflection"][0], 0] *= -1.0
    wp[ROWS["three_live"][0], 3:] = 0.0                          # exactly three live points
    wl[ROWS["three_live"][0]] = 0.0
    wp[ROWS["two_live"][0], 2:] = 0.0                            # two: SINGULAR
    wl[ROWS["two_live"][0]] = 0.0
    row = ROWS["behind"][0]
    t0[row, 2] = -(kw["pts_3d"][row, 0] @ R0[row].T)[2] - 0.1
    wl[ROWS["negative_weight"][0], 4] = -0.5
    return d["K"], R0, t0, kw, wp, wl, status


def test_problems_of_a_batch_do_not_see_each_other(rb):
    K, R0, t0, kw, wp, wl, status = _unlike(rb)
    Kd = _dev(K)

    def run(rows):
        rows = np.asarray(rows)
        res = rb.refine_pose_batch_robust(_dev(R0[rows]), _dev(t0[rows]), K=Kd, loss="cauchy", scale_px=2.0, weights_pts=_dev(wp[rows]),
                                          weights_lines=_dev(wl[rows]), status=_dev(status[rows]), max_iters=UNLIKE_MAX_ITERS,
                                          **{k: _dev(v[rows]) for k, v in kw.items()})
        return _np_result(res)

    full = run(np.arange(12))
    host = rb.refine_pose_batch_robust_host(R0, t0, K=K, loss="cauchy", scale_px=2.0, weights_pts=wp, weights_lines=wl, status=status,
                                            max_iters=UNLIKE_MAX_ITERS, **kw)
    _compare(full, host, R0, t0, "twelve unlike problems")
    st = full.status
    assert st[ROWS["not_admitted"][0]] == st[ROWS["nan_pose"][0]] == st[ROWS["reflection"][0]] == 2
    assert st[ROWS["two_live"][0]] == 3 and st[ROWS["behind"][0]] == 4 and st[ROWS["negative_weight"][0]] == 4
    assert st[ROWS["three_live"][0]] <= 1 and full.n_live[ROWS["three_live"][0]] == 3
    assert st[ROWS["one_trial"][0]] == 0 and full.iters[ROWS["one_trial"][0]] == 1
    assert ((st == 1) & (full.iters == UNLIKE_MAX_ITERS)).any(), (st, full.iters)          # max_iters exhausted
    assert (st[list(ROWS["contaminated"])] <= 1).all()
    perm = np.array([7, 2, 9, 4, 11, 0, 5, 10, 3, 8, 1, 6])
    shuffled = run(perm)
    for b in range(12):
        alone = run([b])
        where = int(np.nonzero(perm == b)[0][0])
        for f in ("R", "t", "cost", "iters", "status", "n_live", "robust_w", "n_inlier"):
            one = getattr(alone, f)[0].tobytes()
            assert one == getattr(full, f)[b].tobytes(), (b, f)
            assert one == getattr(shuffled, f)[where].tobytes(), (b, f)
