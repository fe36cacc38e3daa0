"""Robust PnP for a set of frames with a hypothesis budget PER SCENE: 36 synthetic scenes of 100 correspondences whose share of clutter
runs from 0 to 60 %.  With confidence=0.99 every scene stops as soon as the standard rule says it has drawn enough minimal sets for its
own inlier share; n_hyp = 1024 is only the cap (cvxpnpl_amd.ransac.ransac_pnp_batch(confidence=...); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, CAP = 36, 1024
shares = np.linspace(0.0, 0.6, F)
frames = [synth.make_ransac(1, n_corr=100, outlier_frac=float(s), sigma=0.5, seed=400 + f) for f, s in enumerate(shares)]
out = ransac.ransac_pnp_batch([d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames], synth.K_KINECT, n_hyp=CAP, thresh=2.0, seed=1,
                              confidence=0.99, round_hyp=64, device=torch.device("cuda:0"))
used = out["hyp_used"].numpy()
R, inl, off = out["R"].cpu().numpy(), out["inliers"].cpu().numpy(), out["offsets"].cpu().numpy()
worst = 0.0
for f, d in enumerate(frames):
    mine, truth = inl[off[f]:off[f + 1]], d["inlier"]
    gap = float(synth.geodesic(R[f][None], d["R_gt"][None])[0])
    worst = max(worst, gap)
    assert int(out["n_inliers"][f]) == mine.sum() >= 0.9 * truth.sum() and (mine & ~truth).sum() <= 2 and gap < 2e-2, (f, mine.sum(), truth.sum(), gap)
    assert used[f] % 64 == 0 and 64 <= used[f] <= CAP, (f, used[f])
assert used[0] == 64 and used[:6].max() == 64            # clean scenes stop after the first round
assert used[-1] > used[0] and used.sum() < F * CAP // 2   # cluttered scenes draw more; the set draws a fraction of the fixed budget
print(f"{F} frames, {int(used.sum())} hypotheses solved in {out['rounds']} rounds instead of {F * CAP} (per scene {used.min()} .. {used.max()}), "
      f"worst rotation error {worst:.2e} rad")
