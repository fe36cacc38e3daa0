"""Gradients through the solve AND the refinement: a few Adam steps on the pixels of noisy PnP problems, on the pose a user judges.

pnp_batch_diff -> refine_pose_batch_diff is one connected graph: a converged refinement is differentiated at its reprojection minimum
(the implicit-function VJP with the full Hessian, in HIP), a pose that passed through the refinement hands its gradient to the solve's
backward.  The loss is |R - R_gt|^2 + |t - t_gt|^2 of the REFINED pose; 40 Adam steps of 0.05 px on the pixels bring its mean down.
GPU box:  python examples/refine_grad.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch_diff, refine_pose_batch_diff, synth  # noqa: E402

dev = torch.device("cuda:0")
d = synth.make_pnp(1000, 10, sigma=2.0, seed=11)
x = torch.as_tensor(d["pts_2d"], device=dev).clone().requires_grad_()
X, K, R_gt, t_gt = (torch.as_tensor(d[k], device=dev) for k in ("pts_3d", "K", "R_gt", "t_gt"))
opt = torch.optim.Adam([x], lr=0.05)
steps = 40
for it in range(steps + 1):
    R0, t0, st0 = pnp_batch_diff(x, X, K, certified_only=False)
    R, t, status = refine_pose_batch_diff(R0, t0, pts_2d=x, pts_3d=X, K=K, status=st0)
    loss = ((R - R_gt) ** 2).sum((1, 2)) + ((t - t_gt) ** 2).sum(1)
    err = loss.detach().sqrt().mean().item()
    if it % 10 == 0:
        print(f"step {it:2d}: mean pose error {err:.3e}, refinement converged {(status == 0).float().mean().item():.3f}")
    if it == 0:
        first = err
    if it == steps:
        break
    opt.zero_grad()
    loss.sum().backward()
    opt.step()
assert err < 0.8 * first, (first, err)
print(f"pose error of the refined pose {first:.3e} -> {err:.3e}")
