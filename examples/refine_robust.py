"""Pose polish from raw matches, no mask: 8 synthetic frames of 100 points + 50 lines, 30 % of them clutter, 1 px noise, each started 0.02 rad
and 2 % off its true pose (a tracker's prior).  refine_pose_batch_robust under the Huber loss at 2 px keeps the clutter from pulling --
the least-squares polish of the same records (loss="l2") is dragged away -- and reports per record how much it counted
(cvxpnpl_amd.refine_robust; not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import refine_pose_batch_robust, synth

B, dev = 8, torch.device("cuda:0")
frames = [synth.make_ransac_pnpl(100, 50, outlier_frac=0.3, sigma=1.0, seed=500 + f) for f in range(B)]
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
R_gt = np.stack([d["R_gt"] for d in frames])

plain = refine_pose_batch_robust(R0, t0, loss="l2", max_iters=100, **data)
huber = refine_pose_batch_robust(R0, t0, loss="huber", scale_px=2.0, max_iters=100, **data)
assert (plain.status <= 1).all() and (huber.status == 0).all()
err = [synth.geodesic(o.R.cpu().numpy(), R_gt) for o in (plain, huber)]
assert err[1].max() < 5e-3 and (err[1] * 10.0 < err[0]).all()                     # the known answer: the true pose, to the noise
inlier = np.stack([np.concatenate([d["inlier_pts"], d["inlier_lines"]]) for d in frames])
w = huber.robust_w.cpu().numpy()
assert np.median(w[inlier]) == 1.0 and np.median(w[~inlier]) < 0.1
n_in, truth = huber.n_inlier.cpu().numpy(), inlier.sum(1)
assert (n_in > 0.65 * truth).all() and (n_in <= truth + 5).all()
print(f"{B} frames, 150 raw matches each, 30 % clutter: rotation error {np.mean(synth.geodesic(R0.cpu().numpy(), R_gt)):.1e} rad at the start, "
      f"{err[0].mean():.1e} after the least-squares polish, {err[1].mean():.1e} under the Huber loss ({huber.iters.double().mean():.1f} trials); "
      f"median weight of the clutter {np.median(w[~inlier]):.3f}, records within 2 px {int(n_in.sum())} of {int(truth.sum())} true inliers")
