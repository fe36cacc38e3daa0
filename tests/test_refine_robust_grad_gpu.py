"""refine_robust_vjp_group_kernel<RPL> against the host path (the same source, csrc/refine_robust_vjp_core.h; only the order of the sums
differs): relative 1e-10 per problem over all six gradients, the bound of tests/test_refine_grad_gpu.py.  The shapes are the smallest
at which a layout can go wrong: B = 1, 3, 4, 5 (an empty, a partial and a full last wavefront of four problems), n = 3, 16, 17, 32, 33,
64, 65 records (either side of the RPL = 1 / 2 / 4 switches, and the re-reading kernel with one record on a second pass), points only,
lines only and mixed, each under l2 / Huber / Cauchy, with and without weights, unmasked and with every third record masked and spoiled;
then a camera per problem, a strided status column, subsets of the gradients (the weights' alone among them), unlike neighbours, bad
weights and the saddle.

The two paths differ in the order of their sums and in what the compiler fuses, an error of a few eps that the 6x6 solve amplifies by
the reciprocal of its smallest pivot ratio (info[:, 1]).  1e-10 is the bar for problems whose pivot ratio is at least PIVOT_MIN = 1e-4
(50 eps / 1e-4 = 1e-10), which converged() asserts of the HOST path alone for every problem it hands out; the seeds are ones for which
that holds (a minimal 3-line problem can have a pivot ratio of 1e-6: SEEDS)."""
import functools

import numpy as np
import pytest
import torch

import refine_grad_cases as gc
import refine_robust_grad_cases as rc
import refine_robust_grad_reference as rr

pytestmark = pytest.mark.gpu

BOUND = 1e-10
ADMIT = 0x3   # converged and max_iters: a minimal problem may stop at either
SIZES = ((3, 0), (16, 0), (17, 0), (32, 0), (33, 0), (64, 0), (65, 0), (0, 3), (0, 16), (0, 17), (0, 32), (0, 33), (0, 64), (0, 65),
         (2, 1), (9, 7), (10, 7), (20, 12), (20, 13), (40, 24), (40, 25))
LOSSES = ("l2", "huber", "cauchy")
PIVOT_MIN = 1e-4
SEEDS = {(0, 3): 47}   # (the default, 41 + 3 n_p + n_l = 44, holds a 3-line problem with a pivot ratio of 1e-6)


@functools.lru_cache(maxsize=None)
def converged(n_p, n_l, loss, weights=True, masked=False, batch=5, K_per=False):
    """A batch at the host robust refinement's poses.  Returns (K, R, t, refine status, kw, w, masks, GR, gt, loss)."""
    from cvxpnpl_amd.refine_robust import refine_pose_batch_robust_host

    K, R0, t0, kw, w, GR, gt = rc.shaped(n_p, n_l, batch, seed=SEEDS.get((n_p, n_l), 41 + 3 * n_p + n_l), weights=weights)
    if K_per:
        K = np.stack([K * np.array([[1.0 + 0.01 * b], [1.0 - 0.005 * b], [1.0]]) for b in range(batch)])
    masks = {"mask_pts": None, "mask_lines": None}
    if masked:
        keep = np.ones(n_p + n_l, np.uint8)
        keep[2::3] = 0
        masks = {"mask_pts": np.tile(keep[:n_p], (batch, 1)) if n_p else None, "mask_lines": np.tile(keep[n_p:], (batch, 1)) if n_l else None}
        kw = gc.spoiled(kw, masks)
    res = refine_pose_batch_robust_host(R0, t0, K=K, loss=loss, scale_px=1.0, max_iters=100, **kw, **w, **masks)
    h = run_host(K, res.R, res.t, res.status, kw, w, masks, GR, gt, loss)
    assert (h["info"][h["vjp_status"] == 0, 1] >= PIVOT_MIN).all(), (n_p, n_l, loss, weights, masked, h["info"][:, 1])
    return K, res.R, res.t, res.status, kw, w, masks, GR, gt, loss


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def run_device(K, R, t, status, kw, w, masks, GR, gt, loss, rows=None, **opts):
    from cvxpnpl_amd.refine_robust_grad import refine_vjp_robust

    sl = slice(None) if rows is None else rows
    cut = lambda x: None if x is None else dev(x[sl])  # noqa: E731
    opts.setdefault("admit_mask", ADMIT)
    out = refine_vjp_robust(cut(R), cut(t), cut(status), cut(GR), cut(gt), K=dev(K[sl] if np.ndim(K) == 3 else K), loss=loss, scale_px=1.0,
                            want_info=True, **{k: cut(v) for k, v in kw.items()}, **{k: cut(v) for k, v in w.items()},
                            **{k: cut(v) for k, v in masks.items()}, **opts)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def run_host(K, R, t, status, kw, w, masks, GR, gt, loss, **opts):
    from cvxpnpl_amd.refine_robust_grad import refine_vjp_robust_host

    opts.setdefault("admit_mask", ADMIT)
    return refine_vjp_robust_host(R, t, status, GR, gt, K=K, loss=loss, scale_px=1.0, **kw, **w, **masks, **opts)


def compare(d, h, rows, minimal=False):
    """device result d (of the problems `rows` of the batch) against the host result h of the whole batch; minimal: three records, an
    exact fit, where |g| and its scale are both rounding noise and their ratio -- on either side anything from 0 to 1 -- says nothing"""
    worst = 0.0
    for i, b in enumerate(rows):
        assert d["vjp_status"][i] == h["vjp_status"][b], (b, d["vjp_status"], h["vjp_status"])
        worst = max(worst, rr.rel_err(rr.flat(d, i), rr.flat(h, b)))
        if h["vjp_status"][b] != 0:
            assert not np.any(rr.flat(d, i)), b
        hi, di = h["info"][b], d["info"][i]
        assert np.array_equal(np.isnan(hi), np.isnan(di)), (b, hi, di)
        if not np.isnan(hi).any():
            assert abs(di[1] - hi[1]) <= 1e-6 * hi[1], (b, hi, di)
            if not minimal:
                assert abs(di[0] - hi[0]) <= 1e-12, (b, hi, di)
    return worst


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("size", SIZES)
def test_device_matches_host(size, loss):
    worst = 0.0
    for weights in (True, False):
        for masked in (False, True):
            case = converged(*size, loss, weights=weights, masked=masked)
            h = run_host(*case)
            if sum(size) > 4:                                        # (a minimal problem masked is singular)
                assert (h["vjp_status"] == 0).all(), (weights, masked, h["vjp_status"])
            for B in (1, 3, 4, 5):                                   # an empty, a partial and a full last wavefront
                rows = list(range(5 - B, 5))
                d = run_device(*case, rows=rows)
                for k in rr.NAMES:
                    assert (d[k] is None) == (h[k] is None), k
                    if d[k] is not None:
                        assert np.isfinite(d[k]).all(), k            # every element written
                worst = max(worst, compare(d, h, rows, minimal=sum(size) <= 3))
            if masked:
                for names, m in ((("pts_2d", "pts_3d", "weights_pts"), "mask_pts"), (("line_2d", "line_3d", "weights_lines"), "mask_lines")):
                    if case[6][m] is not None:
                        off = case[6][m] == 0
                        for k in names:
                            assert not np.any(d[k][off]), k          # exactly zero where not live
    print(f"{size} {loss}: device against host {worst:.2e}")
    assert worst <= BOUND


def test_camera_per_problem_strided_status_and_gradient_subsets():
    from cvxpnpl_amd.refine_robust_grad import refine_vjp_robust

    case = converged(9, 7, "huber", K_per=True)
    K, R, t, status, kw, w, masks, GR, gt, loss = case
    h = run_host(*case)
    d = run_device(*case)
    assert compare(d, h, range(5)) <= BOUND
    assert np.abs(rr.flat(d, 1) - rr.flat(run_device(converged(9, 7, "huber")[0], *case[1:]), 1)).max() > 0       # K[b] is read, not K[0]
    # a status column of a wider table, with statuses that are not admitted
    table = torch.full((5, 4), 7, dtype=torch.int32, device="cuda")
    st = np.array([0, 1, 0, 2, 0], np.int32)
    table[:, 2] = dev(st)
    col = table[:, 2]
    assert col.stride(0) == 4
    args = dict(K=dev(K), loss=loss, scale_px=1.0, **{k: dev(v) for k, v in kw.items()}, **{k: dev(v) for k, v in w.items()})
    out = refine_vjp_robust(dev(R), dev(t), col, dev(GR), dev(gt), **args)
    hs = run_host(K, R, t, st, kw, w, masks, GR, gt, loss, admit_mask=0x1)
    assert out["vjp_status"].cpu().numpy().tolist() == hs["vjp_status"].tolist() == [0, 1, 0, 1, 0]
    ds = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    for b in range(5):
        assert rr.rel_err(rr.flat(ds, b), rr.flat(hs, b)) <= BOUND
    out = refine_vjp_robust(dev(R), dev(t), col, dev(GR), dev(gt), admit_mask=0x2, **args)
    assert out["vjp_status"].cpu().numpy().tolist() == [1, 0, 1, 1, 1]
    # subsets: the others' pointers are null, what is returned is the same bytes
    for want in (("weights_pts", "weights_lines"), ("weights_lines",), ("pts_2d",), ("line_3d", "weights_pts"), ("pts_3d", "line_2d"), ()):
        sub = run_device(*case, want=want)
        for k in rr.NAMES:
            if k in want:
                assert sub[k].tobytes() == d[k].tobytes(), (want, k)
            else:
                assert sub[k] is None
        assert sub["vjp_status"].tolist() == d["vjp_status"].tolist()
    # the weights' gradients with the weights absent: the derivative at w = 1
    nw = {"weights_pts": None, "weights_lines": None}
    ones = {"weights_pts": np.ones((5, 9)), "weights_lines": np.ones((5, 7))}
    a, z = run_device(K, R, t, status, kw, nw, masks, GR, gt, loss), run_device(K, R, t, status, kw, ones, masks, GR, gt, loss)
    assert a["weights_pts"] is not None and rr.flat(a).tobytes() == rr.flat(z).tobytes()
    # missing upstream gradients count as zero
    a = run_device(K, R, t, status, kw, w, masks, None, gt, loss)
    z = run_device(K, R, t, status, kw, w, masks, np.zeros_like(GR), gt, loss)
    assert rr.flat(a).tobytes() == rr.flat(z).tobytes()


def unlike_batch():
    """12 problems of (6 points, 4 lines) under the Cauchy loss, four to a wavefront, with every vjp_status among them.  Returns the
    arguments of run_* and the expected statuses."""
    K, R, t, status, kw, w, masks, GR, gt, loss = converged(6, 4, "cauchy", batch=12)
    R, t, status, GR = R.copy(), t.copy(), status.copy(), GR.copy()
    kw, w = {k: v.copy() for k, v in kw.items()}, {k: v.copy() for k, v in w.items()}
    mp, ml = np.ones((12, 6), np.uint8), np.ones((12, 4), np.uint8)
    expect = np.zeros(12, np.int32)
    status[1] = 2                                                # not admitted
    expect[1] = 1
    R[2, 0] = -R[2, 0]                                           # det R < 0
    expect[2] = 1
    mp[3, 1:] = 0                                                # two live records
    ml[3, 1:] = 0
    expect[3] = 2
    w["weights_pts"][4, 1] = -0.5                                # a negative weight on an admitted record
    expect[4] = 3
    Y = kw["pts_3d"][5, 2] @ R[5].T                              # a record behind the camera
    t[5, 2] = -Y[2] - 0.1
    expect[5] = 3
    kw["line_2d"][6, 3, 0, 1] = np.nan                           # NaN in a live record
    expect[6] = 3
    w["weights_pts"][7, ::2] = 0.0                               # zero weights over garbage beside live records
    kw["pts_2d"][7, ::2] = np.nan
    kw["pts_3d"][7, ::2] = 1e9
    t[8] = np.inf                                                # a non-finite pose
    expect[8] = 1
    kw["line_2d"][9, 0, 1] = kw["line_2d"][9, 0, 0]              # a line with a = b
    GR[10, 1, 1] = np.nan                                        # a non-finite upstream gradient
    expect[10] = 3
    w["weights_lines"][11, 2] = np.nan                           # a NaN weight behind a zero mask byte: ignored
    ml[11, 2] = 0
    return (K, R, t, status, kw, w, {"mask_pts": mp, "mask_lines": ml}, GR, gt, loss), expect


def test_unlike_neighbours_do_not_touch_each_other():
    case, expect = unlike_batch()
    h = run_host(*case)
    assert h["vjp_status"].tolist() == expect.tolist(), (h["vjp_status"], expect)
    d = run_device(*case)
    assert compare(d, h, range(12)) <= BOUND
    assert not np.any(d["weights_pts"][7, ::2]) and np.all(d["weights_pts"][7, 1::2] != 0.0)
    perm = np.array([7, 2, 11, 0, 5, 9, 3, 10, 1, 8, 6, 4])
    p = run_device(*case, rows=perm)
    for i, b in enumerate(perm):
        alone = run_device(*case, rows=[b])
        for k in rr.NAMES + ("vjp_status", "info"):
            assert alone[k][0].tobytes() == d[k][b].tobytes() == p[k][i].tobytes(), (b, k)


def test_bad_weights_and_the_saddle_on_the_device():
    from cvxpnpl_amd.refine_robust_grad import refine_vjp_robust

    case = converged(9, 7, "huber")
    K, R, t, status, kw, w, masks, GR, gt, loss = case
    for bad in (-1.0, np.nan, np.inf):
        wb = {k: v.copy() for k, v in w.items()}
        wb["weights_lines"][2, 6] = bad
        d = run_device(K, R, t, status, kw, wb, masks, GR, gt, loss)
        assert d["vjp_status"].tolist() == [0, 0, 3, 0, 0] and not np.any(rr.flat(d, 2)) and np.isnan(d["info"][2]).all(), bad
        ml = np.ones((5, 7), np.uint8)
        ml[2, 6] = 0
        d = run_device(K, R, t, status, kw, wb, {"mask_pts": None, "mask_lines": ml}, GR, gt, loss)
        assert d["vjp_status"].tolist() == [0] * 5 and np.isfinite(rr.flat(d)).all(), bad
    s = rc.saddle()
    out = refine_vjp_robust(dev(s["R"]), dev(s["t"]), None, dev(s["GR"]), dev(s["gt"]), K=dev(s["K"]), loss="cauchy", scale_px=1.0, want_info=True,
                            **{k: dev(v) for k, v in s["kw"].items()})
    assert out["vjp_status"].cpu().tolist() == [2]
    assert not out["line_2d"].any() and not out["line_3d"].any() and not out["weights_lines"].any() and out["pts_2d"] is None
    assert float(out["info"][0, 0]) < 1e-10
