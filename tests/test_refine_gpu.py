"""The refinement kernels of the batch form (cvxpnpl_refine_batch: refine_group_kernel<1|2|4|0>, cov_group_kernel) against the host path of
the same source (cvxpnpl_refine_batch_host) and against the independent reference's next step (tests/refine_reference.py)."""
import numpy as np
import pytest
import torch

import refine_cases as rc

pytestmark = pytest.mark.gpu
B = 130  # not a multiple of 4: the last wavefront has empty groups
# (n_p, n_l, sigma): 1 record per lane; points and lines; lines only; 2 per lane with a ragged tail; the 4-per-lane kernel; the re-reading kernel
SHAPES = ((10, 0, 1.0), (5, 5, 1.0), (0, 6, 1.0), (17, 0, 2.0), (33, 7, 1.0), (70, 0, 1.0))


def _dev(x, dtype=torch.float64):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda")


def _np(res):
    return type(res)(*[None if x is None else x.cpu().numpy() for x in res])


def _run_both(R0, t0, K, kw, **opts):
    from cvxpnpl_amd import refine as rf

    host = rf.refine_pose_batch_host(R0, t0, K=K, **opts, **kw)
    dkw = {k: _dev(v, torch.uint8 if k.startswith("mask") else torch.float64) for k, v in kw.items()}
    if "status" in opts:
        opts = dict(opts, status=_dev(opts["status"], torch.int32))
    dev = _np(rf.refine_pose_batch(_dev(R0), _dev(t0), K=_dev(K), **opts, **dkw))
    return host, dev


@pytest.mark.parametrize("per_problem_K", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_host_and_is_stationary(shape, per_problem_K):
    n_p, n_l, sigma = shape
    d, R0, t0, kw = rc.problem(B, n_p, n_l, sigma)
    K = d["K"]
    if per_problem_K:
        K = np.tile(K, (B, 1, 1))
        K[:, 0, 0] *= 1.0 + 0.01 * np.arange(B) / B      # (the 2D data were made with the shared K: the problems differ a little, which is the point)
    host, dev = _run_both(R0, t0, K, kw, max_iters=100)
    assert dev.status.tolist() == host.status.tolist() and (dev.status == 0).all()
    assert dev.n_live.tolist() == host.n_live.tolist()
    same = float((dev.iters == host.iters).mean())
    print(f"{shape} per_problem_K={per_problem_K}: iters equal for {100 * same:.1f} %, max {dev.iters.max()}")
    assert same >= 0.95
    assert (dev.cost[:, 1] <= dev.cost[:, 0]).all()
    assert np.abs(dev.cost[:, 0] - host.cost[:, 0]).max() <= 1e-9 * host.cost[:, 0].max()
    rows = range(0, B, 5) if per_problem_K else range(B)    # (the reference is slow: every problem once, a sample the second time)
    worst = rc.worst_next_step(K, dev.R, dev.t, kw, rows=rows)
    print(f"   reference's next step from the device's poses <= {worst:.2e}")
    assert worst <= rc.STEP_BAR
    assert np.abs(dev.R - host.R).max() <= rc.STEP_BAR and np.abs(dev.t - host.t).max() <= rc.STEP_BAR


def test_edge_cases_in_one_wavefront():
    K, R0, t0, kw, status_in, masks, expect = rc.edge_batch()
    host, dev = _run_both(R0, t0, K, dict(kw, **masks), status=status_in, max_iters=100, want_cov=True)
    rc.check_edge_batch(dev, R0, t0, expect)
    assert dev.status.tolist() == host.status.tolist() and dev.n_live.tolist() == host.n_live.tolist()
    live = np.nonzero(expect < 2)[0]
    assert rc.worst_next_step(K, dev.R, dev.t, kw, rows=live, masks=masks) <= rc.STEP_BAR


@pytest.mark.parametrize("shape", [(10, 0, 1.0), (5, 5, 1.0), (70, 0, 1.0)])
@pytest.mark.parametrize("sigma_px", [0.0, 1.5])
def test_covariance_on_the_device(shape, sigma_px):
    n_p, n_l, sigma = shape
    d, R0, t0, kw = rc.problem(24, n_p, n_l, sigma)
    host, dev = _run_both(R0, t0, d["K"], kw, max_iters=100, want_cov=True, sigma_px=sigma_px)
    assert (dev.status == 0).all()
    worst = rc.worst_cov_ratio(d["K"], dev, kw, sigma_px)
    print(f"{shape} sigma_px={sigma_px}: covariance error / bound <= {worst:.3f}")
    assert worst <= 1.0


def test_status_column_and_in_place_output():
    """A strided status column is read as it is (head[:, 0] of the RANSAC read-back), admit_mask selects, and the outputs may be the
    inputs' own arrays."""
    from cvxpnpl_amd import refine as rf

    d, R0, t0, kw = rc.problem(9, 10, 0, 1.0)
    head = torch.zeros((9, 4), dtype=torch.int32, device="cuda")
    head[:, 1] = 7                                             # (what a wrong stride would read)
    head[2, 0], head[5, 0] = 1, 2
    res = rf.refine_pose_batch(_dev(R0), _dev(t0), pts_2d=_dev(kw["pts_2d"]), pts_3d=_dev(kw["pts_3d"]), K=_dev(d["K"]), status=head[:, 0])
    st = res.status.cpu().numpy()
    assert st[2] == 2 and (np.delete(st, 2) <= 1).all()
    # in place: the C entry with d_R_out = d_R and d_t_out = d_t (the Python wrapper always allocates), the same strided column
    import ctypes as C

    from cvxpnpl_amd import _lib

    def ptr(x):
        return C.c_void_p(x.data_ptr())

    R, t, p2, p3, K = _dev(R0), _dev(t0), _dev(kw["pts_2d"]), _dev(kw["pts_3d"]), _dev(d["K"])
    _, _, cost, iters, ost, n_live, _ = rf._outputs(9, R.device, False)
    code = _lib.refine_lib().cvxpnpl_refine_batch(9, 10, ptr(p2), ptr(p3), 0, None, None, ptr(K), 0, ptr(R), ptr(t), ptr(head), 4, rf.ADMIT_USABLE, None, None,
                                                  None, ptr(R), ptr(t), ptr(cost), ptr(iters), ptr(ost), ptr(n_live), None,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0
    for got, want in ((R, res.R), (t, res.t), (cost, res.cost), (iters, res.iters), (ost, res.status), (n_live, res.n_live)):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert R[2].cpu().numpy().tobytes() == R0[2].tobytes() and t[2].cpu().numpy().tobytes() == t0[2].tobytes()   # the skipped one: bit for bit
    res = rf.refine_pose_batch(_dev(R0), _dev(t0), pts_2d=_dev(kw["pts_2d"]), pts_3d=_dev(kw["pts_3d"]), K=_dev(d["K"]), status=head[:, 0], admit_mask=0x1)
    assert res.status.cpu().numpy()[[2, 5]].tolist() == [2, 2]


def test_start_from_the_solver_s_own_poses():
    """pnp_batch at sigma = 1: the algebraic minimiser is a good start, and the refinement does not make its pixel error worse."""
    from cvxpnpl_amd import pnp_batch, refine as rf, synth

    d = synth.make_pnp(B, 10, 1.0, seed=11)
    p2, p3, K = _dev(d["pts_2d"]), _dev(d["pts_3d"]), _dev(d["K"])
    sol = pnp_batch(p2, p3, K)
    res = rf.refine_pose_batch(sol.R, sol.t, pts_2d=p2, pts_3d=p3, K=K, status=sol.status)
    st, cost, sst = res.status.cpu().numpy(), res.cost.cpu().numpy(), sol.status.cpu().numpy()
    usable = np.isin(sst, (0, 2))
    assert usable.mean() > 0.9 and (st[~usable] == 2).all() and np.isin(st[usable], (0, 1, 4)).all()
    done = st <= 1
    assert done.mean() > 0.9 and (cost[done, 1] <= cost[done, 0]).all()
    rms0, rms1 = np.sqrt(cost[done, 0] / 20.0), np.sqrt(cost[done, 1] / 20.0)
    print(f"rms pixel error, algebraic {rms0.mean():.4f} -> refined {rms1.mean():.4f}; mean trials {res.iters.cpu().numpy()[done].mean():.2f}")
    assert (rms1 <= rms0).all()
