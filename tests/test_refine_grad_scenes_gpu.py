"""refine_vjp_scenes_kernel (packed scenes of different sizes, masks, one workgroup of 256 per scene) against the batch host path on each
scene alone, relative 1e-10 as in tests/test_refine_grad_gpu.py: 3, 255, 256 and 257 points (one thread short of, exactly, and one past a
workgroup), 0, 1 and 50 lines, consensus-style masks with garbage in what they leave out, one scene fully masked; and the same scenes
in reversed order, byte-identical per scene."""
import functools

import numpy as np
import pytest
import torch

import refine_grad_cases as gc
import refine_grad_reference as rg

pytestmark = pytest.mark.gpu

BOUND = 1e-10
SIZES = ((3, 1), (255, 0), (256, 50), (257, 0), (9, 50))   # (a packed scene holds at least four correspondences: 3 points go with 1 line)


@functools.lru_cache(maxsize=None)
def scenes():
    """Five scenes at the host refinement's converged poses.  Returns a list of (K, R [1,3,3], t, refine status, kw, masks, GR, gt), batch 1
    each; scene 2 carries a consensus-style mask over spoiled records, scene 3 is fully masked."""
    from cvxpnpl_amd.refine import refine_pose_batch_host

    out = []
    for f, (n_p, n_l) in enumerate(SIZES):
        K, R0, t0, kw, GR, gt = gc.shaped(n_p, n_l, 1, seed=79 + f)   # (seeds at which the minimal scene converges)
        K = K * np.array([[1.0 + 0.01 * f], [1.0 - 0.005 * f], [1.0]])       # a camera per scene
        if n_l == 0:
            kw = dict(kw, line_2d=np.zeros((1, 0, 2, 2)), line_3d=np.zeros((1, 0, 2, 3)))
        masks = {"mask_pts": np.ones((1, n_p), np.uint8), "mask_lines": np.ones((1, n_l), np.uint8)}
        if f == 2:
            masks["mask_pts"][0, ::3] = 0
            masks["mask_lines"][0, 1::4] = 0
            kw = gc.spoiled(kw, masks)
        if f == 3:
            masks["mask_pts"][:] = 0
        if f == 4:
            masks["mask_pts"][0, 5:] = 0
        res = refine_pose_batch_host(R0, t0, K=K, max_iters=100, **kw, **masks)
        out.append((K, res.R, res.t, res.status, kw, masks, GR, gt))
    return out


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def run_scenes(order):
    from cvxpnpl_amd import ransac as rn
    from cvxpnpl_amd.refine_grad import refine_vjp_scenes

    ss = [scenes()[f] for f in order]
    cat = lambda i, k=None: np.concatenate([(s[i] if k is None else s[i][k]) for s in ss])  # noqa: E731
    sc = rn.pack_pnpl_scenes([s[4]["pts_2d"][0] for s in ss], [s[4]["line_2d"][0] for s in ss], [s[4]["pts_3d"][0] for s in ss],
                             [s[4]["line_3d"][0] for s in ss], np.stack([s[0] for s in ss]), device="cuda")
    mp = dev(np.concatenate([s[5]["mask_pts"][0] for s in ss]))
    ml = dev(np.concatenate([s[5]["mask_lines"][0] for s in ss]))
    out = refine_vjp_scenes(sc, dev(cat(1)), dev(cat(2)), dev(cat(3)), dev(cat(6)), dev(cat(7)), mask_pts=mp, mask_lines=ml, want_info=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    # cut the packed gradients back into scenes
    op = np.concatenate([[0], np.cumsum([SIZES[f][0] for f in order])])
    ol = np.concatenate([[0], np.cumsum([SIZES[f][1] for f in order])])
    per = {}
    for i, f in enumerate(order):
        per[f] = {"pts_2d": out["pts_2d"][op[i]:op[i + 1]], "pts_3d": out["pts_3d"][op[i]:op[i + 1]], "line_2d": out["line_2d"][ol[i]:ol[i + 1]],
                  "line_3d": out["line_3d"][ol[i]:ol[i + 1]], "vjp_status": out["vjp_status"][i], "info": out["info"][i]}
    return per


def test_scenes_match_the_host_per_scene_and_do_not_depend_on_their_order():
    from cvxpnpl_amd.refine_grad import refine_vjp_host

    fwd = run_scenes(range(len(SIZES)))
    expect = [0, 0, 0, 1, 0]                                       # the fully masked scene was not refined (status 3): skipped
    worst = 0.0
    for f, (K, R, t, st, kw, masks, GR, gt) in enumerate(scenes()):
        h = refine_vjp_host(R, t, st, GR, gt, K=K, **kw, **masks)
        assert fwd[f]["vjp_status"] == h["vjp_status"][0] == expect[f], (f, fwd[f]["vjp_status"], h["vjp_status"])
        got = np.concatenate([fwd[f][k].reshape(-1) for k in rg.NAMES])
        want = np.concatenate([(h[k][0].reshape(-1) if h[k] is not None else np.zeros(0)) for k in rg.NAMES])
        assert got.shape == want.shape and np.isfinite(got).all(), f
        err = rg.rel_err(got, want)
        worst = max(worst, err)
        for k2, k3, m in (("pts_2d", "pts_3d", "mask_pts"), ("line_2d", "line_3d", "mask_lines")):
            off = masks[m][0] == 0
            assert not np.any(fwd[f][k2][off]) and not np.any(fwd[f][k3][off]), (f, k2)      # exactly zero where not live
        if expect[f]:
            assert not np.any(got), f
        else:
            assert np.any(got), f
            assert abs(fwd[f]["info"][1] - h["info"][0, 1]) <= 1e-6 * h["info"][0, 1], (f, fwd[f]["info"], h["info"][0])
            if h["info"][0, 0] < 1e-3:   # (at an exact fit |g| and its scale are both rounding noise)
                assert abs(fwd[f]["info"][0] - h["info"][0, 0]) <= 1e-12, (f, fwd[f]["info"], h["info"][0])
    print(f"scenes against the host, worst {worst:.2e}")
    assert worst <= BOUND
    rev = run_scenes(list(reversed(range(len(SIZES)))))
    for f in range(len(SIZES)):
        for k in rg.NAMES + ("vjp_status", "info"):
            assert np.asarray(rev[f][k]).tobytes() == np.asarray(fwd[f][k]).tobytes(), (f, k)


def test_point_scenes_without_lines_and_a_strided_status():
    """ransac.Scenes (no line arrays at all), shared K, statuses read from a column of a wider table, a subset of the gradients."""
    from cvxpnpl_amd import ransac as rn
    from cvxpnpl_amd.refine_grad import refine_vjp_host, refine_vjp_scenes

    ss = [scenes()[f] for f in (1, 3, 4)]
    K = scenes()[0][0]
    sc = rn.pack_scenes([s[4]["pts_2d"][0] for s in ss], [s[4]["pts_3d"][0] for s in ss], K, device="cuda")
    R, t = np.concatenate([s[1] for s in ss]), np.concatenate([s[2] for s in ss])
    GR, gt = np.concatenate([s[6] for s in ss]), np.concatenate([s[7] for s in ss])
    table = torch.full((3, 3), 9, dtype=torch.int32, device="cuda")
    table[:, 0] = torch.tensor([0, 1, 0], dtype=torch.int32)
    out = refine_vjp_scenes(sc, dev(R), dev(t), table[:, 0], dev(GR), dev(gt), want=("pts_3d",))
    assert out["pts_2d"] is None and out["line_2d"] is None and out["line_3d"] is None
    assert out["vjp_status"].cpu().tolist() == [0, 1, 0]
    g = out["pts_3d"].cpu().numpy()
    o = np.cumsum([0, 255, 257, 9])
    for i, s in enumerate(ss):
        h = refine_vjp_host(R[i:i + 1], t[i:i + 1], np.array([[0, 1, 0][i]], np.int32), GR[i:i + 1], gt[i:i + 1], K=K, pts_2d=s[4]["pts_2d"],
                            pts_3d=s[4]["pts_3d"])
        assert rg.rel_err(g[o[i]:o[i + 1]].reshape(-1), h["pts_3d"].reshape(-1)) <= BOUND, i
    assert not np.any(g[o[1]:o[2]])
