"""refine_vjp_group_kernel<RPL> against the host path (the same source, csrc/refine_vjp_core.h; only the order of the sums differs):
relative 1e-10 per problem over all gradients, the bound of tests/test_pose_grad_gpu.py.  The shapes are the smallest at which a layout
can go wrong: B = 1, 3, 4, 5 (an empty, a partial and a full last wavefront of four problems), n = 3, 16, 17, 64, 65 records (one record
per lane, either side of the RPL = 1 / 2 / 4 switches, and the re-reading kernel with one record on a second pass), points only, lines
only and mixed, every third record masked and spoiled, a camera per problem, a strided status column, subsets of the gradients."""
import functools

import numpy as np
import pytest
import torch

import refine_grad_cases as gc
import refine_grad_reference as rg

pytestmark = pytest.mark.gpu

BOUND = 1e-10
SHAPES = ((3, 0), (16, 0), (17, 0), (64, 0), (65, 0), (0, 3), (0, 16), (0, 17), (0, 64), (0, 65), (9, 7), (10, 7), (20, 12), (40, 24), (40, 25))


@functools.lru_cache(maxsize=None)
def converged(n_p, n_l, batch=5, masked=False, K_per=False):
    """A batch at the host refinement's converged poses (with the masks, when masked).  Returns (K, R, t, refine status, kw, masks, GR, gt)."""
    from cvxpnpl_amd.refine import refine_pose_batch_host

    K, R0, t0, kw, GR, gt = gc.shaped(n_p, n_l, batch, seed=41 + 3 * n_p + n_l)
    if K_per:
        K = np.stack([K * np.array([[1.0 + 0.01 * b], [1.0 - 0.005 * b], [1.0]]) for b in range(batch)])
    masks = {"mask_pts": None, "mask_lines": None}
    if masked:
        keep = np.ones(n_p + n_l, np.uint8)
        keep[2::3] = 0
        masks = {"mask_pts": np.tile(keep[:n_p], (batch, 1)) if n_p else None, "mask_lines": np.tile(keep[n_p:], (batch, 1)) if n_l else None}
        kw = gc.spoiled(kw, masks)
    res = refine_pose_batch_host(R0, t0, K=K, max_iters=100, **kw, **masks)
    return K, res.R, res.t, res.status, kw, masks, GR, gt


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def run_device(K, R, t, status, kw, masks, GR, gt, rows=None, **opts):
    from cvxpnpl_amd.refine_grad import refine_vjp

    sl = slice(None) if rows is None else rows
    cut = lambda x: None if x is None else dev(x[sl])  # noqa: E731
    out = refine_vjp(cut(R), cut(t), cut(status), cut(GR), cut(gt), K=dev(K[sl] if np.ndim(K) == 3 else K), want_info=True,
                     **{k: cut(v) for k, v in kw.items()}, **{k: cut(v) for k, v in masks.items()}, **opts)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def run_host(K, R, t, status, kw, masks, GR, gt, **opts):
    from cvxpnpl_amd.refine_grad import refine_vjp_host

    return refine_vjp_host(R, t, status, GR, gt, K=K, **kw, **masks, **opts)


def compare(d, h, rows):
    """device result d (of the problems `rows` of the batch) against the host result h of the whole batch"""
    worst = 0.0
    for i, b in enumerate(rows):
        assert d["vjp_status"][i] == h["vjp_status"][b], (b, d["vjp_status"], h["vjp_status"])
        worst = max(worst, rg.rel_err(rg.flat(d, i), rg.flat(h, b)))
        if h["vjp_status"][b] != 0:
            assert not np.any(rg.flat(d, i)), b
        hi, di = h["info"][b], d["info"][i]
        assert np.array_equal(np.isnan(hi), np.isnan(di)), (b, hi, di)
        if not np.isnan(hi).any():
            assert abs(di[1] - hi[1]) <= 1e-6 * hi[1], (b, hi, di)
            if hi[0] < 1e-3:   # (at an exact fit -- the minimal problems -- |g| and its scale are both rounding noise: their ratio says nothing)
                assert abs(di[0] - hi[0]) <= 1e-12, (b, hi, di)
    return worst


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_matches_host(shape, masked):
    case = converged(*shape, masked=masked)
    h = run_host(*case)
    if sum(shape) > 4:                                               # (a minimal problem may end max_iters, and masked it is singular)
        assert (h["vjp_status"] == 0).all(), h["vjp_status"]
    elif not masked:
        assert (h["vjp_status"] == 0).sum() >= 3, h["vjp_status"]
    worst = 0.0
    for B in (1, 3, 4, 5):                                           # an empty, a partial and a full last wavefront
        rows = list(range(5 - B, 5))
        d = run_device(*case, rows=rows)
        for k in rg.NAMES:
            assert (d[k] is None) == (h[k] is None)
            if d[k] is not None:
                assert np.isfinite(d[k]).all(), k                        # every element written
        worst = max(worst, compare(d, h, rows))
    if masked:
        for k2, k3, m in (("pts_2d", "pts_3d", "mask_pts"), ("line_2d", "line_3d", "mask_lines")):
            if case[5][m] is not None:
                off = case[5][m] == 0
                assert not np.any(d[k2][off]) and not np.any(d[k3][off])   # exactly zero where not live
    print(f"{shape} masked={masked}: device against host {worst:.2e}")
    assert worst <= BOUND


def test_camera_per_problem_strided_status_and_gradient_subsets():
    case = converged(9, 7, K_per=True)
    K, R, t, status, kw, masks, GR, gt = case
    h = run_host(*case)
    d = run_device(*case)
    assert compare(d, h, range(5)) <= BOUND
    assert np.abs(rg.flat(d, 1) - rg.flat(run_device(converged(9, 7)[0], *case[1:]), 1)).max() > 0       # K[b] is read, not K[0]
    # a status column of a wider table, with statuses that are not admitted
    from cvxpnpl_amd.refine_grad import refine_vjp

    table = torch.full((5, 4), 7, dtype=torch.int32, device="cuda")
    st = np.array([0, 1, 0, 2, 0], np.int32)
    table[:, 2] = dev(st)
    col = table[:, 2]
    assert col.stride(0) == 4
    out = refine_vjp(dev(R), dev(t), col, dev(GR), dev(gt), K=dev(K), **{k: dev(v) for k, v in kw.items()})
    hs = run_host(K, R, t, st, kw, masks, GR, gt)
    assert out["vjp_status"].cpu().numpy().tolist() == hs["vjp_status"].tolist() == [0, 1, 0, 1, 0]
    ds = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    for b in range(5):
        assert rg.rel_err(rg.flat(ds, b), rg.flat(hs, b)) <= BOUND
    # admit_mask over the refine status
    out = refine_vjp(dev(R), dev(t), col, dev(GR), dev(gt), K=dev(K), admit_mask=0x2, **{k: dev(v) for k, v in kw.items()})
    assert out["vjp_status"].cpu().numpy().tolist() == [1, 0, 1, 1, 1]
    # subsets: the others' pointers are null, what is returned is the same bytes
    for want in (("pts_2d",), ("line_3d",), ("pts_3d", "line_2d"), ()):
        sub = run_device(*case, want=want)
        for k in rg.NAMES:
            if k in want:
                assert sub[k].tobytes() == d[k].tobytes(), (want, k)
            else:
                assert sub[k] is None
        assert sub["vjp_status"].tolist() == d["vjp_status"].tolist()
    # missing upstream gradients count as zero
    a = run_device(K, R, t, status, kw, masks, None, gt)
    z = run_device(K, R, t, status, kw, masks, np.zeros_like(GR), gt)
    assert rg.flat(a).tobytes() == rg.flat(z).tobytes()


def unlike_batch():
    """12 problems of (6 points, 4 lines), four to a wavefront, with every vjp_status among them.  Returns the arguments of run_* and the
    expected statuses."""
    K, R, t, status, kw, masks, GR, gt = converged(6, 4, batch=12)
    R, t, status, GR = R.copy(), t.copy(), status.copy(), GR.copy()
    kw = {k: v.copy() for k, v in kw.items()}
    mp, ml = np.ones((12, 6), np.uint8), np.ones((12, 4), np.uint8)
    expect = np.zeros(12, np.int32)
    status[1] = 1                                                # not admitted
    expect[1] = 1
    R[2, 0] = -R[2, 0]                                           # det R < 0
    expect[2] = 1
    mp[3, 1:] = 0                                                # two live records
    ml[3, 1:] = 0
    expect[3] = 2
    Y = kw["pts_3d"][5, 2] @ R[5].T                              # a record behind the camera
    t[5, 2] = -Y[2] - 0.1
    expect[5] = 3
    kw["line_2d"][6, 3, 0, 1] = np.nan                           # NaN in a live record
    expect[6] = 3
    mp[7, ::2] = 0                                               # masked records with garbage beside live ones
    kw["pts_2d"][7, ::2] = np.nan
    kw["pts_3d"][7, ::2] = 1e9
    t[8] = np.inf                                                # a non-finite pose
    expect[8] = 1
    kw["line_2d"][9, 0, 1] = kw["line_2d"][9, 0, 0]              # a line with a = b
    GR[10, 1, 1] = np.nan                                        # a non-finite upstream gradient
    expect[10] = 3
    return (K, R, t, status, kw, {"mask_pts": mp, "mask_lines": ml}, GR, gt), expect


def test_unlike_neighbours_do_not_touch_each_other():
    case, expect = unlike_batch()
    h = run_host(*case)
    assert h["vjp_status"].tolist() == expect.tolist(), (h["vjp_status"], expect)
    d = run_device(*case)
    assert compare(d, h, range(12)) <= BOUND
    perm = np.array([7, 2, 11, 0, 5, 9, 3, 10, 1, 8, 6, 4])
    p = run_device(*case, rows=perm)
    for i, b in enumerate(perm):
        alone = run_device(*case, rows=[b])
        for k in rg.NAMES + ("vjp_status", "info"):
            assert alone[k][0].tobytes() == d[k][b].tobytes() == p[k][i].tobytes(), (b, k)


def test_saddle_is_refused_on_the_device():
    s = gc.saddle()
    from cvxpnpl_amd.refine_grad import refine_vjp

    out = refine_vjp(dev(s["R"]), dev(s["t"]), None, dev(s["GR"]), dev(s["gt"]), K=dev(s["K"]), want_info=True,
                     **{k: dev(v) for k, v in s["kw"].items()})
    assert out["vjp_status"].cpu().tolist() == [2]
    assert not out["line_2d"].any() and not out["line_3d"].any() and out["pts_2d"] is None
    assert float(out["info"][0, 0]) < 1e-10
