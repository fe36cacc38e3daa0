"""Robust PnPL for a set of frames in one call: 24 synthetic scenes of 20 .. 300 points and 10 .. 150 lines (the last four: lines only),
30 % of the points and of the lines replaced by clutter, 512 minimal sets of four correspondences per scene drawn from points and lines
together, assembled, solved, scored, selected and refitted on the device (cvxpnpl_amd.ransac.ransac_pnpl_batch; not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

n_pts = [int(v) for v in np.round(np.geomspace(20, 300, 24))]
n_lines = [int(v) for v in np.round(np.geomspace(10, 150, 24))]
n_pts[-4:] = [0, 0, 0, 0]
frames = [synth.make_ransac_pnpl(p, l, outlier_frac=0.3, sigma=0.5, seed=400 + f) for f, (p, l) in enumerate(zip(n_pts, n_lines))]
out = ransac.ransac_pnpl_batch([d["pts_2d"] for d in frames], [d["line_2d"] for d in frames], [d["pts_3d"] for d in frames],
                               [d["line_3d"] for d in frames], synth.K_KINECT, n_hyp=512, thresh=2.0, seed=1, device=torch.device("cuda:0"))
R = out["R"].cpu().numpy()
ip, op, il, ol = out["inliers_pts"].cpu().numpy(), out["offsets"].cpu().numpy(), out["inliers_lines"].cpu().numpy(), out["line_offsets"].cpu().numpy()
worst = 0.0
for f, d in enumerate(frames):
    mp, ml = ip[op[f]:op[f + 1]], il[ol[f]:ol[f + 1]]
    truth = int(d["inlier_pts"].sum() + d["inlier_lines"].sum())
    gap = float(synth.geodesic(R[f][None], d["R_gt"][None])[0])
    worst = max(worst, gap)
    # (a cluttered LINE can pass by chance more easily than a point: two distances to one line instead of a 2D distance)
    assert int(out["n_inliers"][f]) == mp.sum() + ml.sum() >= 0.9 * truth and (mp & ~d["inlier_pts"]).sum() <= 2, (f, mp.sum(), ml.sum(), truth)
    assert (ml & ~d["inlier_lines"]).sum() <= 3 and gap < 2e-2, (f, ml.sum(), gap)
print(f"{len(frames)} frames, {int(out['n_inliers'].sum())} inliers of {op[-1]} points + {ol[-1]} lines, {int(out['n_certified'].sum())} of "
      f"{len(frames) * out['n_hyp']} hypotheses certified, worst rotation error {worst:.2e} rad")
