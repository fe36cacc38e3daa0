"""Adaptive RANSAC over points and lines with local optimisation: 24 synthetic scenes of 100 points and 50 lines, 50 % clutter among
both and 1 px of noise, thresh 2 px, confidence 0.99 under a cap of 1024 hypotheses in rounds of 64.  A pose from four correspondences
explains only part of the true inliers -- a line needs BOTH end points within the threshold, so it is under-counted even more than a
point -- and the stopping rule keeps drawing; local_opt=3 refits every scene's running best on the points and lines near it at the end of
every round (thresholds 2x -> 1x) and lets the refit's count decide -- same draws, fewer of them
(cvxpnpl_amd.ransac.ransac_pnpl_batch(confidence=..., local_opt=..., lo_widen=...); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, CAP = 24, 1024
frames = [synth.make_ransac_pnpl(n_pts=100, n_lines=50, outlier_frac=0.5, sigma=1.0, seed=100 + f) for f in range(F)]
args = tuple([d[k] for d in frames] for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")) + (synth.K_KINECT,)
R_gt = np.stack([d["R_gt"] for d in frames])
kw = dict(n_hyp=CAP, thresh=2.0, seed=0, refit=False, confidence=0.99, round_hyp=64, device=torch.device("cuda:0"))
plain = ransac.ransac_pnpl_batch(*args, **kw)
lo = ransac.ransac_pnpl_batch(*args, local_opt=3, lo_widen=2.0, **kw)
used_p, used_l = plain["hyp_used"].numpy(), lo["hyp_used"].numpy()
assert (used_l <= used_p).all()                                   # no scene draws more: the draws are the same, the running best never lower
assert used_l.sum() <= 0.79 * used_p.sum(), (used_l.sum(), used_p.sum())
assert lo["n_inliers"].double().mean() > plain["n_inliers"].double().mean() and int(lo["lo_taken"].sum()) > 0
n_mask = lo["inliers_pts"].view(F, 100).sum(dim=1) + lo["inliers_lines"].view(F, 50).sum(dim=1)
assert (n_mask.cpu() == lo["n_inliers"]).all()                    # both masks and the count belong to the same pose
err_p = np.degrees(synth.geodesic(plain["R"].cpu().numpy(), R_gt))
err_l = np.degrees(synth.geodesic(lo["R"].cpu().numpy(), R_gt))
print(f"{F} frames under a cap of {CAP}: hypotheses drawn {used_p.sum()} -> {used_l.sum()} (ratio {used_l.sum() / used_p.sum():.2f}), rounds "
      f"{plain['rounds']} -> {lo['rounds']}, mean inliers {plain['n_inliers'].double().mean():.1f} -> {lo['n_inliers'].double().mean():.1f}, "
      f"{int(lo['lo_taken'].sum())} refits taken, mean rotation error {err_p.mean():.3f} -> {err_l.mean():.3f} deg")
