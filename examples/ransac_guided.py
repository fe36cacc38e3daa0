"""Robust PnP guided by the matcher's scores: 24 synthetic scenes of 100 correspondences, 70 % of them clutter, and a budget of only 32
hypotheses per scene.  Uniform draws hit an all-inlier minimal set in about one scene of five at that budget; with quality= the first
hypotheses come from the best-ranked correspondences and nearly every scene is solved (cvxpnpl_amd.ransac.ransac_pnp_batch(quality=...,
pool_full=...); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, H = 24, 32
rs = np.random.RandomState(5)
frames = [synth.make_ransac(1, n_corr=100, outlier_frac=0.7, sigma=0.5, seed=900 + f) for f in range(F)]
# a matcher's confidence that knows something, not everything: inliers score U(0.2, 1), clutter U(0, 0.8)
quality = [np.where(d["inlier"], rs.uniform(0.2, 1.0, 100), rs.uniform(0.0, 0.8, 100)) for d in frames]
args = ([d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames], synth.K_KINECT)
kw = dict(n_hyp=H, thresh=2.0, seed=1, device=torch.device("cuda:0"))
uniform = ransac.ransac_pnp_batch(*args, **kw)
guided = ransac.ransac_pnp_batch(*args, quality=quality, pool_full=1024, **kw)
assert guided["pool_full"] == 1024 and [ransac.pool_size(h, 100, 1024) for h in (0, 1, 16, 1000)] == [4, 5, 20, 100]


def solved(out):
    R, inl, off = out["R"].cpu().numpy(), out["inliers"].cpu().numpy(), out["offsets"].cpu().numpy()
    ok = []
    for f, d in enumerate(frames):
        kept = (inl[off[f]:off[f + 1]] & d["inlier"]).sum()
        gap = float(synth.geodesic(R[f][None], d["R_gt"][None])[0]) if np.isfinite(R[f]).all() else np.inf
        ok.append(2 * kept >= d["inlier"].sum() and gap < 2e-2)
    return np.array(ok)


u, g = solved(uniform), solved(guided)
assert g.sum() >= 0.9 * F and u.sum() <= 0.5 * F, (int(g.sum()), int(u.sum()))
# pool_full = 0 turns the guidance off: the uniform call, bit for bit
off = ransac.ransac_pnp_batch(*args, quality=quality, pool_full=0, **kw)
assert torch.equal(off["R"].view(torch.int64), uniform["R"].view(torch.int64)) and torch.equal(off["inliers"], uniform["inliers"])
print(f"{F} frames of 70 % clutter, {H} hypotheses each: {int(u.sum())} solved with uniform draws, {int(g.sum())} guided by the scores")
