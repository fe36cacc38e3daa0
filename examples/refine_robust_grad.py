"""Learning a matcher's confidences end to end: Adam on per-correspondence log-weights through the refinement.

1 000 PnP problems of 20 points at sigma = 1 px; 30 % of every problem's pixels are displaced by 20-200 px.  The weighted least-squares
refinement (loss "l2": nothing but the weights can switch an outlier off) is differentiated at its minimum by the implicit-function
VJP in HIP, the weights' gradients included (refine_pose_batch_robust_diff), and the loss is |R - R_gt|^2 + |t - t_gt|^2 of the refined
pose.  The weights start at 1 and are parametrised as exp(logit), so that none reaches exactly 0 (a zero weight is a mask and stays 0).
After 60 Adam steps the displaced records' weights have fallen below the clean ones' and the pose error with them.  Measured on one
MI355X: mean pose error 3.68e-1 -> 1.97e-2 (x 0.053), mean weight of the displaced records over that of the clean ones 1 -> 0.122.  The asserted bars are half the measured improvement.
GPU box:  python examples/refine_robust_grad.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import refine_pose_batch_robust_diff, synth  # noqa: E402

WEIGHT_RATIO_BAR = 0.56  # mean weight of the displaced records over that of the clean ones, at the end: below this
ERROR_RATIO_BAR = 0.53   # mean pose error at the end over the one at the start: below this

dev = torch.device("cuda:0")
B, n = 1000, 20
d = synth.make_pnp(B, n, sigma=1.0, seed=21)
rs = np.random.RandomState(22)
displaced = np.zeros((B, n), bool)
x = d["pts_2d"].copy()
for b in range(B):
    idx = rs.choice(n, 6, replace=False)
    displaced[b, idx] = True
    ang, mag = rs.uniform(0.0, 2.0 * np.pi, 6), rs.uniform(20.0, 200.0, 6)
    x[b, idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
x, X, K, R_gt, t_gt = (torch.as_tensor(v, device=dev) for v in (x, d["pts_3d"], d["K"], d["R_gt"], d["t_gt"]))
bad = torch.as_tensor(displaced, device=dev)
logit = torch.zeros((B, n), dtype=torch.float64, device=dev, requires_grad=True)
opt = torch.optim.Adam([logit], lr=0.1)
steps = 60
for it in range(steps + 1):
    w = torch.exp(logit)
    R, t, status = refine_pose_batch_robust_diff(R_gt, t_gt, pts_2d=x, pts_3d=X, K=K, loss="l2", weights_pts=w)
    loss = ((R - R_gt) ** 2).sum((1, 2)) + ((t - t_gt) ** 2).sum(1)
    err = loss.detach().sqrt().mean().item()
    ratio = (w.detach()[bad].mean() / w.detach()[~bad].mean()).item()
    if it % 10 == 0:
        print(f"step {it:2d}: mean pose error {err:.3e}, mean weight displaced / clean {ratio:.3f}, converged {(status == 0).float().mean().item():.3f}")
    if it == 0:
        first = err
    if it == steps:
        break
    opt.zero_grad()
    loss.sum().backward()
    opt.step()
print(f"pose error {first:.3e} -> {err:.3e} (x {err / first:.3f}), mean weight displaced / clean {ratio:.3f}")
assert ratio < WEIGHT_RATIO_BAR, ratio
assert err < ERROR_RATIO_BAR * first, (first, err)
