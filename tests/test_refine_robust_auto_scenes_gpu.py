"""The scenes kernels of the twelfth library -- robust_scale_scenes_kernel, refine_robust_pp_scenes_kernel with robust_w_pp_scenes_kernel,
robust_cov_scenes_kernel: one workgroup of 256 per scene -- against the batch host path on each scene alone and against the seventh
library's scenes call: scenes of 0, 1, 2, 3, 255, 256, 257 and 600 points (nothing, under, at and over one pass of the workgroup, and a
third pass), with and without lines, a shared camera and one per scene, masks and zero weights over spoiled records.

Bars (device against host, those of tests/test_refine_robust_scenes_gpu.py): statuses and counts equal; sq and sigma 1e-8 relative; the
covariance COV_DEVICE_HOST of |V|_F (no reference floor is at hand for these scenes; where it is, tests/test_refine_robust_auto_gpu.py
holds the issue's 100 floors).  Bit for bit: med_sq against numpy.median of the device's own live sq; a uniform scale array against the seventh
library; the automatic call against the explicit calls it stands for."""
import numpy as np
import pytest
import torch

import refine_cases as rc
import refine_robust_auto_reference as ar

pytestmark = pytest.mark.gpu

POINTS = (0, 1, 2, 3, 255, 256, 257, 600)
COV_DEVICE_HOST = 1e-10                       # (tests/test_refine_robust_auto_gpu.py: the same sums in another order, through two solves with H)
LINES = (5, 1, 0, 3, 0, 50, 1, 7)             # with lines: scenes 1 (1 + 1 records) and 2 (2 + 0) stay below three live records


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _scenes(lines):
    out = []
    for f, n_p in enumerate(POINTS):
        n_l = LINES[f] if lines else 0
        d, R0, t0, kw = rc.problem(1, 600, 50, 1.0 + 0.5 * (f % 3), seed=700 + f)
        p2, p3, l2, l3 = kw["pts_2d"][0, :n_p].copy(), kw["pts_3d"][0, :n_p].copy(), kw["line_2d"][0, :n_l].copy(), kw["line_3d"][0, :n_l].copy()
        rs = np.random.RandomState(f)
        n = n_p + n_l
        w, m = rs.uniform(0.1, 2.0, n), np.ones(n, np.uint8)
        if n > 8:
            m[3::4] = 0
            w[4::5] = 0.0
        off = (m == 0) | (w == 0.0)
        p2[off[:n_p]], p3[off[:n_p]] = np.nan, 1e9
        l2[off[n_p:]], l3[off[n_p:]] = np.nan, 1e9
        out.append({"K": d["K"] * np.array([[1.0 + 0.002 * f], [1.0], [1.0]]), "R0": R0[0], "t0": t0[0], "p2": p2, "p3": p3, "l2": l2, "l3": l3, "w": w, "m": m,
                    "n_p": n_p, "n_l": n_l})
    return out


def _pack(rn, scenes, lines, per_scene_K):
    """The packed scene set built field by field (ransac.pack_scenes refuses a scene of fewer than four correspondences)."""
    cat = lambda key: _dev(np.concatenate([s[key] for s in scenes]))  # noqa: E731
    off = lambda key: _dev(np.concatenate([[0], np.cumsum([s[key] for s in scenes])]).astype(np.int64))  # noqa: E731
    K = _dev(np.stack([s["K"] for s in scenes])) if per_scene_K else _dev(scenes[0]["K"])
    sizes, lsizes = [s["n_p"] for s in scenes], [s["n_l"] for s in scenes]
    if lines:
        return rn.PnplScenes(cat("p2"), cat("p3"), cat("l2"), cat("l3"), off("n_p"), off("n_l"), sizes, lsizes, K)
    return rn.Scenes(cat("p2"), cat("p3"), off("n_p"), sizes, K)


def _host_kw(s, K):
    n_p, n_l = s["n_p"], s["n_l"]
    kw = {"K": K}
    if n_p:
        kw.update(pts_2d=s["p2"][None], pts_3d=s["p3"][None], weights_pts=s["w"][None, :n_p].copy(), mask_pts=s["m"][None, :n_p].copy())
    if n_l:
        kw.update(line_2d=s["l2"][None], line_3d=s["l3"][None], weights_lines=s["w"][None, n_p:].copy(), mask_lines=s["m"][None, n_p:].copy())
    return kw


def _per_scene(scenes, pair):
    """a packed per-record pair ([sum P], [sum L] or None) as one array per scene, points then lines"""
    p = pair[0].cpu().numpy()
    l = pair[1].cpu().numpy() if pair[1] is not None else np.zeros(0)
    out, op, ol = [], 0, 0
    for s in scenes:
        out.append(np.concatenate([p[op:op + s["n_p"]], l[ol:ol + s["n_l"]]]))
        op, ol = op + s["n_p"], ol + s["n_l"]
    assert op == len(p) and ol == len(l)
    return out


@pytest.mark.parametrize("per_scene_K", (False, True), ids=("shared-K", "K-per-scene"))
@pytest.mark.parametrize("lines", (False, True), ids=("points", "points-and-lines"))
def test_scenes_equal_the_host_path_scene_by_scene(lines, per_scene_K):
    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    scenes = _scenes(lines)
    F = len(scenes)
    sc = _pack(rn, scenes, lines, per_scene_K)
    R0, t0 = np.stack([s["R0"] for s in scenes]), np.stack([s["t0"] for s in scenes])
    dR, dt = _dev(R0), _dev(t0)
    tens = dict(weights_pts=_dev(np.concatenate([s["w"][:s["n_p"]] for s in scenes])), mask_pts=_dev(np.concatenate([s["m"][:s["n_p"]] for s in scenes])))
    if lines:
        tens.update(weights_lines=_dev(np.concatenate([s["w"][s["n_p"]:] for s in scenes])), mask_lines=_dev(np.concatenate([s["m"][s["n_p"]:] for s in scenes])))

    # 1. the scale
    est = ca.robust_scale_scenes(sc, dR, dt, **tens)
    sq = _per_scene(scenes, est.sq)
    sigma, med, n_live, st = (x.cpu().numpy() for x in (est.sigma_px, est.med_sq, est.n_live, est.status))
    worst = 0.0
    for f, s in enumerate(scenes):
        K = s["K"] if per_scene_K else scenes[0]["K"]
        if s["n_p"] + s["n_l"] == 0:                                # the host's batch form needs a record: an empty scene has no live one
            assert st[f] == 3 and n_live[f] == 0 and np.isnan(sigma[f]) and np.isnan(med[f])
            continue
        h = ca.robust_scale_batch_host(s["R0"][None], s["t0"][None], **_host_kw(s, K))
        assert st[f] == h.status[0] and n_live[f] == h.n_live[0], (f, st[f], h.status[0])
        live = (s["m"] != 0) & (s["w"] != 0.0)
        assert n_live[f] == live.sum()
        if st[f] != 0:
            assert st[f] == 3 and live.sum() < 3 and np.isnan(sq[f]).all() and np.isnan(sigma[f]) and np.isnan(med[f]), f
            continue
        assert (sq[f][~live] == -1.0).all()
        np.testing.assert_allclose(sq[f][live], h.sq[0][live], rtol=1e-8, atol=0.0)
        worst = max(worst, abs(sigma[f] - h.sigma_px[0]) / h.sigma_px[0])
        assert med[f].tobytes() == np.float64(np.median(sq[f][live])).tobytes(), f                 # bit for bit, of the device's own sq
        want = np.sqrt(med[f] / ar.CHI2_2_MEDIAN)
        assert abs(sigma[f] - want) <= 4.0 * np.spacing(want), f
    print(f"sigma within {worst:.1e} of the host's; statuses {st.tolist()}")
    assert worst <= 1e-8
    assert [int(x) for x in st] == ([3, 3, 3, 0, 0, 0, 0, 0] if not lines else [0, 3, 3, 0, 0, 0, 0, 0])

    # 2. the loop: a uniform scale array is the seventh library's scenes call bit for bit; the automatic call is its explicit calls
    for loss in ("huber", "cauchy"):
        want = ca.refine_scenes_robust(sc, dR, dt, loss=loss, scale_px=1.5, **tens)
        got = ca.refine_scenes_robust_auto(sc, dR, dt, loss=loss, scale_px=_dev(np.full(F, 1.5)), **tens)
        for name in ("R", "t", "cost", "iters", "status", "n_live", "n_inlier"):
            assert getattr(got, name).cpu().numpy().tobytes() == getattr(want, name).cpu().numpy().tobytes(), (loss, name)
        for a, b in zip(got.robust_w, want.robust_w):
            assert (a is None and b is None) or a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), loss
    auto = ca.refine_scenes_robust_auto(sc, dR, dt, loss="huber", covariance=True, **tens)
    scale = torch.clamp(est.sigma_px * ca.refine_robust_auto.SCALE_FACTOR_95, min=1e-3)
    step = ca.refine_scenes_robust_auto(sc, dR, dt, loss="huber", scale_px=scale, **tens)
    ast = auto.status.cpu().numpy()
    ok = ast <= 1
    assert ast.tolist() == st.tolist() or (ast[st == 0] <= 1).all() and (ast[st != 0] == st[st != 0]).all()
    for name in ("R", "t", "cost", "iters", "n_inlier"):
        assert getattr(auto, name).cpu().numpy()[ok].tobytes() == getattr(step, name).cpu().numpy()[ok].tobytes(), name
    assert auto.R.cpu().numpy()[~ok].tobytes() == R0[~ok].tobytes() and auto.t.cpu().numpy()[~ok].tobytes() == t0[~ok].tobytes()   # bit for bit
    assert auto.scale_px.cpu().numpy()[ok].tobytes() == scale.cpu().numpy()[ok].tobytes() and np.isnan(auto.scale_px.cpu().numpy()[~ok]).all()

    # 3. the covariance: the functional form on the result, and the host path scene by scene
    cov = ca.robust_covariance_scenes(sc, auto.R, auto.t, loss="huber", scale_px=auto.scale_px, status=auto.status, **tens)
    acov, cst = auto.cov.cpu().numpy(), cov.status.cpu().numpy()
    assert cov.cov.cpu().numpy().tobytes() == acov.tobytes()
    aR, at, asc = auto.R.cpu().numpy(), auto.t.cpu().numpy(), auto.scale_px.cpu().numpy()
    rel = 0.0
    for f, s in enumerate(scenes):
        if not ok[f]:
            assert cst[f] == 2 and np.isnan(acov[f]).all(), f
            continue
        K = s["K"] if per_scene_K else scenes[0]["K"]
        h = ca.robust_covariance_host(aR[f][None], at[f][None], loss="huber", scale_px=np.array([asc[f]]), **_host_kw(s, K))
        assert cst[f] == h.status[0], (f, cst[f], h.status[0])
        if cst[f] == 0:
            rel = max(rel, np.linalg.norm(acov[f] - h.cov[0]) / np.linalg.norm(h.cov[0]))
        else:
            assert np.isnan(acov[f]).all()
    print(f"covariance within {rel:.1e} of the host's, relative to |V|_F; statuses {cst.tolist()}")
    assert rel <= COV_DEVICE_HOST and (cst[4:] == 0).all()


def test_bad_scenes_between_good_ones_l2_and_outputs_on_the_input_pose():
    """Six scenes of 40 points + 10 lines, every fourth record masked and spoiled: scene 1 is not admitted (status 2), scene 3 has a bad
    weight (4), scene 4 lies behind the camera (4), and the scale array gives scene 2 a NaN (4).  The good scenes equal the seventh
    library's scenes call bit for bit, the bad ones pass through bit for bit; l2 does not read the scale array; and the outputs of
    cvxpnpl_refine_robust_pp_scenes may alias the input pose."""
    import ctypes as C

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import _lib, ransac as rn
    from cvxpnpl_amd.api import _ptr

    scenes = []
    for f in range(6):
        d, R0, t0, kw = rc.problem(1, 40, 10, 1.0, seed=760 + f)
        p2, p3, l2, l3 = (kw[k][0].copy() for k in ("pts_2d", "pts_3d", "line_2d", "line_3d"))
        w, m = np.ones(50), np.ones(50, np.uint8)
        m[3::4] = 0
        off = m == 0
        p2[off[:40]], p3[off[:40]], l2[off[40:]], l3[off[40:]] = np.nan, 1e9, np.nan, 1e9
        scenes.append({"K": d["K"], "R0": R0[0], "t0": t0[0].copy(), "p2": p2, "p3": p3, "l2": l2, "l3": l3, "w": w, "m": m, "n_p": 40, "n_l": 10})
    scenes[3]["w"][0] = -1.0
    scenes[4]["t0"] = -scenes[4]["t0"]
    F = len(scenes)
    sc = _pack(rn, scenes, True, False)
    R0, t0 = np.stack([s["R0"] for s in scenes]), np.stack([s["t0"] for s in scenes])
    status = np.array([0, 1, 0, 0, 0, 0], np.int32)
    tens = dict(weights_pts=_dev(np.concatenate([s["w"][:40] for s in scenes])), mask_pts=_dev(np.concatenate([s["m"][:40] for s in scenes])),
                weights_lines=_dev(np.concatenate([s["w"][40:] for s in scenes])), mask_lines=_dev(np.concatenate([s["m"][40:] for s in scenes])),
                status=_dev(status), admit_mask=1)
    dR, dt = _dev(R0), _dev(t0)
    est = ca.robust_scale_scenes(sc, dR, dt, **tens)
    assert est.status.cpu().numpy().tolist() == [0, 2, 0, 4, 4, 0]
    sig = est.sigma_px.cpu().numpy()
    assert np.isfinite(sig[[0, 2, 5]]).all() and np.isnan(sig[[1, 3, 4]]).all()
    for f in (0, 2, 5):                                              # the neighbours of the bad ones are what they are alone
        h = ca.robust_scale_batch_host(R0[f][None], t0[f][None], **_host_kw(scenes[f], scenes[f]["K"]))
        assert abs(sig[f] - h.sigma_px[0]) <= 1e-8 * h.sigma_px[0]
    np_ = lambda x: x.cpu().numpy()  # noqa: E731
    scale = np.full(F, 1.5)
    scale[2] = np.nan
    for loss in ("l2", "huber", "cauchy"):
        want = ca.refine_scenes_robust(sc, dR, dt, loss=loss, scale_px=1.5, **tens)
        got = ca.refine_scenes_robust_auto(sc, dR, dt, loss=loss, scale_px=_dev(scale), covariance=True, **tens)
        wst, gst = np_(want.status), np_(got.status)
        assert wst.tolist() == [wst[0], 2, wst[2], 4, 4, wst[5]] and (wst[[0, 2, 5]] <= 1).all()
        bad2 = loss != "l2"                                          # l2 does not read the array: its NaN is nothing
        assert gst.tolist() == [wst[0], 2, 4 if bad2 else wst[2], 4, 4, wst[5]], (loss, gst)
        keep = np.array([True, True, not bad2, True, True, True])
        for name in ("R", "t", "cost", "iters", "n_live", "n_inlier"):
            assert np_(getattr(got, name))[keep].tobytes() == np_(getattr(want, name))[keep].tobytes(), (loss, name)
        gw, ww = _per_scene(scenes, got.robust_w), _per_scene(scenes, want.robust_w)
        for f in range(F):
            if keep[f]:
                assert gw[f].tobytes() == ww[f].tobytes(), (loss, f)
            else:
                assert np.isnan(gw[f]).all()
        failed = gst > 1
        assert np_(got.R)[failed].tobytes() == R0[failed].tobytes() and np_(got.t)[failed].tobytes() == t0[failed].tobytes()      # bit for bit
        cst = np_(got.cov_status)
        assert (cst[failed] == 2).all() and (cst[~failed] == 0).all() and np.isnan(np_(got.cov)[failed]).all() and np.isfinite(np_(got.cov)[~failed]).all()

    # the outputs on the input pose, through the C entry point
    want = ca.refine_scenes_robust_auto(sc, dR, dt, loss="huber", scale_px=_dev(scale), **tens)
    R, t, dsc = _dev(R0), _dev(t0), _dev(scale)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    cost, rwp, rwl = torch.empty((F, 2), **f64), torch.zeros((sc.total,), **f64), torch.zeros((sc.line_total,), **f64)
    iters, ost, n_live, n_in = (torch.empty((F,), **i32) for _ in range(4))
    L = _lib.refine_robust_auto_lib()
    o = _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), 30, 1e-10, 1e-3, _lib.LOSS_HUBER, 1.0)
    rc_ = L.cvxpnpl_refine_robust_pp_scenes(F, _ptr(sc.offsets), sc.total, _ptr(sc.line_offsets), sc.line_total, _ptr(sc.x), _ptr(sc.X), _ptr(sc.l2), _ptr(sc.l3),
                                            _ptr(sc.K), 0, _ptr(R), _ptr(t), _ptr(tens["status"]), 1, 1, _ptr(tens["mask_pts"]), _ptr(tens["mask_lines"]),
                                            _ptr(tens["weights_pts"]), _ptr(tens["weights_lines"]), _ptr(dsc), C.byref(o), _ptr(R), _ptr(t), _ptr(cost),
                                            _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rwp), _ptr(rwl), _ptr(n_in), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, L.cvxpnpl_refine_robust_auto_last_error()
    torch.cuda.synchronize()
    assert np_(ost).tolist() == np_(want.status).tolist() == [np_(ost)[0], 2, 4, 4, 4, np_(ost)[5]]
    assert np_(R).tobytes() == np_(want.R).tobytes() and np_(t).tobytes() == np_(want.t).tobytes()       # (the failed ones: their input pose)
    ok = np_(ost) <= 1
    assert np_(cost)[ok].tobytes() == np_(want.cost)[ok].tobytes() and np_(iters).tobytes() == np_(want.iters).tobytes()
    assert np_(rwp).tobytes() == np_(want.robust_w[0]).tobytes() and np_(rwl).tobytes() == np_(want.robust_w[1]).tobytes()
