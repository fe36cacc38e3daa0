"""Four frames with four noise levels in one call: 100 points + 50 lines each, 30 % of them gross clutter, pixel noise of 0.5, 1, 2 and 4 px,
each started 0.02 rad and 2 % off its true pose.  refine_pose_batch_robust_auto estimates every frame's sigma from the median squared
residual, polishes each at its own scale (Cauchy, two rounds of estimate-then-polish) and returns the covariance of each pose; the same
call at the single hand-set scale of 1 px is right for one frame and throws away the inliers of the noisy ones
(cvxpnpl_amd.refine_robust_auto; not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import refine_pose_batch_robust_auto, synth

SIGMAS, dev = (0.5, 1.0, 2.0, 4.0), torch.device("cuda:0")
frames = [synth.make_ransac_pnpl(100, 50, outlier_frac=0.3, sigma=s, seed=910 + f) for f, s in enumerate(SIGMAS)]
rs = np.random.RandomState(1)
R0, t0 = [], []
for d in frames:
    w = rs.normal(size=3)
    w *= 0.02 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    R0.append((np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th**2 * W @ W) @ d["R_gt"])
    t0.append(d["t_gt"] * (1.0 + 0.02 * rs.uniform(-1.0, 1.0, 3)))
stack = lambda k: torch.as_tensor(np.stack([d[k] for d in frames]), device=dev)  # noqa: E731
data = dict(pts_2d=stack("pts_2d"), pts_3d=stack("pts_3d"), line_2d=stack("line_2d"), line_3d=stack("line_3d"), K=torch.as_tensor(synth.K_KINECT, device=dev))
R0, t0 = torch.as_tensor(np.stack(R0), device=dev), torch.as_tensor(np.stack(t0), device=dev)
R_gt, t_gt = np.stack([d["R_gt"] for d in frames]), np.stack([d["t_gt"] for d in frames])


def distance(o):
    return synth.geodesic(o.R.cpu().numpy(), R_gt) + np.linalg.norm(o.t.cpu().numpy() - t_gt, axis=1) / np.linalg.norm(t_gt, axis=1)


auto = refine_pose_batch_robust_auto(R0, t0, loss="cauchy", scale_rounds=2, covariance=True, max_iters=100, **data)
fixed = refine_pose_batch_robust_auto(R0, t0, loss="cauchy", scale_px=1.0, max_iters=100, **data)
assert (auto.status <= 1).all() and (fixed.status <= 1).all()
sigma = auto.sigma_px.cpu().numpy()
assert ((sigma < 1.5 * np.array(SIGMAS)) & (sigma * 1.5 > np.array(SIGMAS))).all(), sigma      # (with 30 % clutter the median sits at the inliers' 71st percentile: 1.34 sigma)
da, df = distance(auto), distance(fixed)
assert (da < df).all(), (da, df)                                                              # the known answer: the true pose
sd_t = np.sqrt(np.diagonal(auto.cov.cpu().numpy(), axis1=1, axis2=2)[:, 3:].sum(1))
assert np.isfinite(sd_t).all() and sd_t[3] > sd_t[0]                                          # the noisiest frame reports a wider covariance than the cleanest
print(f"4 frames at sigma = {SIGMAS} px, 30 % clutter: estimated sigma {np.round(sigma, 2).tolist()} px, polished at {np.round(auto.scale_px.cpu().numpy(), 2).tolist()} px; "
      f"distance from the true pose {np.round(da * 1e3, 2).tolist()}e-3 (at the single scale 1 px: {np.round(df * 1e3, 2).tolist()}e-3); "
      f"reported standard deviation of t {np.round(sd_t * 1e3, 2).tolist()}e-3")
