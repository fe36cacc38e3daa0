"""Robust PnP for a set of frames in one call: 36 synthetic scenes of 40 .. 600 correspondences, 30 % of the pixels replaced by
clutter, 512 four-point hypotheses per scene sampled, solved, scored, selected and refitted together on the device
(cvxpnpl_amd.ransac.ransac_pnp_batch; not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

sizes = [int(v) for v in np.round(np.geomspace(40, 600, 36))]
frames = [synth.make_ransac(1, n_corr=m, outlier_frac=0.3, sigma=0.5, seed=200 + f) for f, m in enumerate(sizes)]
out = ransac.ransac_pnp_batch([d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames], synth.K_KINECT, n_hyp=512, thresh=2.0, seed=1,
                              device=torch.device("cuda:0"))
R, inl, off = out["R"].cpu().numpy(), out["inliers"].cpu().numpy(), out["offsets"].cpu().numpy()
worst = 0.0
for f, d in enumerate(frames):
    mine, truth = inl[off[f]:off[f + 1]], d["inlier"]
    gap = float(synth.geodesic(R[f][None], d["R_gt"][None])[0])
    worst = max(worst, gap)
    assert int(out["n_inliers"][f]) == mine.sum() >= 0.9 * truth.sum() and (mine & ~truth).sum() <= 2 and gap < 2e-2, (f, mine.sum(), truth.sum(), gap)
print(f"{len(frames)} frames, {int(out['n_inliers'].sum())} inliers of {off[-1]} correspondences, {int(out['n_certified'].sum())} of "
      f"{len(frames) * out['n_hyp']} hypotheses certified, worst rotation error {worst:.2e} rad")
