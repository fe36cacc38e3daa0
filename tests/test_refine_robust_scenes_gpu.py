"""refine_robust_scenes_kernel / robust_w_scenes_kernel (packed scenes of different sizes, weights and masks, one workgroup per scene)
against the batch host path on each scene alone, in both orders of the scenes, and from the result of a RANSAC run.

Bars (device against host): statuses, n_live, n_inlier equal; poses 1e-8; costs 1e-9 relative; robust_w 1e-8."""
import numpy as np
import pytest
import torch

import refine_cases as rc

pytestmark = pytest.mark.gpu

SIZES = ((3, 1), (255, 0), (256, 50), (257, 0), (9, 50), (8, 4))   # records per scene: under, at and over one pass of the workgroup; the last is switched off
DELTA = 1.5


def _scenes():
    """The six scenes with random weights in [0.1, 2]; every fourth record masked off and spoiled, every fifth at weight 0 and spoiled;
    every weight of the last scene 0."""
    out = []
    for f, (n_p, n_l) in enumerate(SIZES):
        d, R0, t0, kw = rc.problem(1, n_p, n_l, 1.0, seed=80 + f)
        kw = {k: (None if v is None else v[0].copy()) for k, v in kw.items()}
        rs = np.random.RandomState(f)
        w, m = rs.uniform(0.1, 2.0, n_p + n_l), np.ones(n_p + n_l, np.uint8)
        if n_p + n_l > 4:
            m[3::4] = 0
            w[4::5] = 0.0
        if f == len(SIZES) - 1:
            w[:] = 0.0
        off = (m == 0) | (w == 0.0)
        for key2, key3, sel in (("pts_2d", "pts_3d", off[:n_p]), ("line_2d", "line_3d", off[n_p:])):
            if kw[key2] is not None:
                kw[key2][sel] = np.nan
                kw[key3][sel] = 1e9
        out.append({"K": d["K"] * np.array([[1.0 + 0.002 * f], [1.0], [1.0]]), "R0": R0[0], "t0": t0[0], "kw": kw, "w": w, "m": m, "n_p": n_p, "n_l": n_l})
    return out


def _run(rb, rn, scenes, loss):
    sc = rn.pack_pnpl_scenes([s["kw"]["pts_2d"] for s in scenes], [s["kw"]["line_2d"] for s in scenes], [s["kw"]["pts_3d"] for s in scenes],
                             [s["kw"]["line_3d"] for s in scenes], np.stack([s["K"] for s in scenes]), device="cuda")
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    res = rb.refine_scenes_robust(sc, dev(np.stack([s["R0"] for s in scenes])), dev(np.stack([s["t0"] for s in scenes])), loss=loss, scale_px=DELTA,
                                  weights_pts=dev(np.concatenate([s["w"][:s["n_p"]] for s in scenes])),
                                  weights_lines=dev(np.concatenate([s["w"][s["n_p"]:] for s in scenes])),
                                  mask_pts=dev(np.concatenate([s["m"][:s["n_p"]] for s in scenes])),
                                  mask_lines=dev(np.concatenate([s["m"][s["n_p"]:] for s in scenes])), max_iters=100)
    R, t, cost, iters, st, n_live, (rwp, rwl), n_in = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in res]
    rwp, rwl = rwp.cpu().numpy(), rwl.cpu().numpy()
    per, op, ol = [], 0, 0
    for f, s in enumerate(scenes):                                 # per scene: the outputs, robust_w as points then lines
        per.append({"R": R[f], "t": t[f], "cost": cost[f], "iters": iters[f], "status": st[f], "n_live": n_live[f], "n_inlier": n_in[f],
                    "robust_w": np.concatenate([rwp[op:op + s["n_p"]], rwl[ol:ol + s["n_l"]]])})
        op, ol = op + s["n_p"], ol + s["n_l"]
    assert op == len(rwp) and ol == len(rwl)
    return per


@pytest.mark.parametrize("loss", ["l2", "huber", "cauchy"])
def test_scenes_equal_the_host_path_in_both_orders(loss):
    from cvxpnpl_amd import ransac as rn, refine_robust as rb

    scenes = _scenes()
    per = _run(rb, rn, scenes, loss)
    worst = {"pose": 0.0, "cost": 0.0, "w": 0.0}
    for f, (s, o) in enumerate(zip(scenes, per)):
        n_p, kw = s["n_p"], {k: (None if v is None else v[None]) for k, v in s["kw"].items()}
        h = rb.refine_pose_batch_robust_host(s["R0"][None], s["t0"][None], K=s["K"], loss=loss, scale_px=DELTA, max_iters=100,
                                             weights_pts=s["w"][None, :n_p].copy() if n_p else None, weights_lines=s["w"][None, n_p:].copy() if s["n_l"] else None,
                                             mask_pts=s["m"][None, :n_p] if n_p else None, mask_lines=s["m"][None, n_p:] if s["n_l"] else None, **kw)
        assert o["status"] == h.status[0] and o["n_live"] == h.n_live[0] and o["n_inlier"] == h.n_inlier[0], (f, o["status"], h.status[0])
        live = (s["m"] != 0) & (s["w"] != 0.0)
        assert h.n_live[0] == live.sum()
        if f == len(scenes) - 1:
            assert o["status"] == 3                                # every weight 0: no live record
        if h.status[0] <= 1:
            worst["pose"] = max(worst["pose"], np.abs(o["R"] - h.R[0]).max(), np.abs(o["t"] - h.t[0]).max())
            worst["cost"] = max(worst["cost"], (np.abs(o["cost"] - h.cost[0]) / np.abs(h.cost[0])).max())
            worst["w"] = max(worst["w"], np.abs(o["robust_w"] - h.robust_w[0]).max())
            assert (o["robust_w"][~live] == 0.0).all() and (o["robust_w"][live] > 0.0).all()
        else:
            assert o["R"].tobytes() == s["R0"].tobytes() and o["t"].tobytes() == s["t0"].tobytes() and np.isnan(o["cost"]).all()
            assert np.isnan(o["robust_w"]).all() and o["n_inlier"] == 0 and o["iters"] == 0
    print(f"{loss}: poses within {worst['pose']:.1e}, costs within {worst['cost']:.1e}, robust_w within {worst['w']:.1e}")
    assert worst["pose"] <= 1e-8 and worst["cost"] <= 1e-9 and worst["w"] <= 1e-8, worst
    assert all(int(o["status"]) <= 1 for o in per[:-1])
    back = _run(rb, rn, scenes[::-1], loss)[::-1]                  # the same scenes packed in reversed order: byte-identical per scene
    for f, (a, b) in enumerate(zip(per, back)):
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (f, k)


def test_polish_of_a_ransac_result_over_all_records_without_a_mask():
    """The documented use: the RANSAC poses, every record of every scene, no mask, status = head[:, 0] (a strided column)."""
    from cvxpnpl_amd import ransac as rn, refine_robust as rb, synth

    ds = [synth.make_ransac_pnpl(100 + 20 * f, 50, outlier_frac=0.3, sigma=1.0, seed=60 + f) for f in range(3)]
    K = ds[0]["K"]
    args = ([d["pts_2d"] for d in ds], [d["line_2d"] for d in ds], [d["pts_3d"] for d in ds], [d["line_3d"] for d in ds], K)
    out = rn.ransac_pnpl_batch(*args, n_hyp=64, seed=3, device="cuda")
    head = out["head"].to("cuda")
    sc = rn.pack_pnpl_scenes(*args, device="cuda")
    res = rb.refine_scenes_robust(sc, out["R"], out["t"], loss="huber", scale_px=2.0, status=head[:, 0])
    st, hs = res.status.cpu().numpy(), out["head"].numpy()[:, 0]
    solved = np.isin(hs, (0, 2))
    assert solved.all() and np.isin(st[solved], (0, 1)).all(), (hs, st)
    cost, n_live, n_in = res.cost.cpu().numpy(), res.n_live.cpu().numpy(), res.n_inlier.cpu().numpy()
    assert (cost[:, 1] <= cost[:, 0]).all()
    assert n_live.tolist() == [150 + 20 * f for f in range(3)]                             # every record of the scene took part
    truth = np.array([int(d["inlier_pts"].sum() + d["inlier_lines"].sum()) for d in ds])
    print(f"n_inlier {n_in.tolist()} of {n_live.tolist()} (RANSAC consensus {out['n_inliers'].tolist()}, true inliers {truth.tolist()})")
    assert (n_in >= 0.7 * truth).all() and (n_in < n_live).all()    # (at sigma = 1 px and delta = 2 px, 1 - e^-2 = 86 % of the true inliers have s <= delta^2)
    rwp = res.robust_w[0].cpu().numpy()
    off = np.concatenate([[0], np.cumsum([100 + 20 * f for f in range(3)])])
    for f, d in enumerate(ds):                                     # the clutter is weighted down, the true inliers are not
        w = rwp[off[f]:off[f + 1]]
        assert np.median(w[d["inlier_pts"]]) == 1.0 and np.median(w[~d["inlier_pts"]]) < 0.1, f
