"""Adaptive RANSAC with local optimisation: 24 synthetic scenes of 100 correspondences, 50 % clutter and 1 px of noise, thresh 2 px,
confidence 0.99 under a cap of 1024 hypotheses in rounds of 64.  A four-point pose explains only part of the true inliers, so the
stopping rule sees too low an inlier share and keeps drawing; local_opt=3 refits every scene's running best on its consensus set at the
end of every round (thresholds 2x -> 1x) and lets the refit's count decide -- same draws, fewer of them
(cvxpnpl_amd.ransac.ransac_pnp_batch(confidence=..., local_opt=..., lo_widen=...); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, CAP = 24, 1024
frames = [synth.make_ransac(1, n_corr=100, outlier_frac=0.5, sigma=1.0, seed=100 + f) for f in range(F)]
xs, Xs = [d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames]
R_gt = np.stack([d["R_gt"] for d in frames])
kw = dict(n_hyp=CAP, thresh=2.0, seed=0, refit=False, confidence=0.99, round_hyp=64, device=torch.device("cuda:0"))
plain = ransac.ransac_pnp_batch(xs, Xs, synth.K_KINECT, **kw)
lo = ransac.ransac_pnp_batch(xs, Xs, synth.K_KINECT, local_opt=3, lo_widen=2.0, **kw)
used_p, used_l = plain["hyp_used"].numpy(), lo["hyp_used"].numpy()
assert (used_l <= used_p).all()                                   # no scene draws more: the draws are the same, the running best never lower
assert used_l.sum() <= 0.81 * used_p.sum(), (used_l.sum(), used_p.sum())
assert lo["n_inliers"].double().mean() > plain["n_inliers"].double().mean() and int(lo["lo_taken"].sum()) > 0
err_p = np.degrees(synth.geodesic(plain["R"].cpu().numpy(), R_gt))
err_l = np.degrees(synth.geodesic(lo["R"].cpu().numpy(), R_gt))
print(f"{F} frames under a cap of {CAP}: hypotheses drawn {used_p.sum()} -> {used_l.sum()} (ratio {used_l.sum() / used_p.sum():.2f}), rounds "
      f"{plain['rounds']} -> {lo['rounds']}, mean inliers {plain['n_inliers'].double().mean():.1f} -> {lo['n_inliers'].double().mean():.1f}, "
      f"{int(lo['lo_taken'].sum())} refits taken, mean rotation error {err_p.mean():.3f} -> {err_l.mean():.3f} deg")
