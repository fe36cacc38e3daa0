"""Gradients through the batched solve: recover the pixels of 1 000 noisy PnP problems by gradient descent on a pose loss.

The loss is |R - R_gt|^2 + |t - t_gt|^2 per problem; its gradient with respect to the pixels comes from pnp_batch_diff's backward
(the implicit-function VJP of the certified pose, in HIP).  30 steps with a Polyak step size per problem (the loss is 0 at the true
pixels) bring the mean pose error down by more than ten-fold.  GPU box:  python examples/pose_grad.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch_diff, synth  # noqa: E402

dev = torch.device("cuda:0")
d = synth.make_pnp(1000, 10, sigma=2.0, seed=11)
x = torch.as_tensor(d["pts_2d"], device=dev).clone().requires_grad_()
X, K, R_gt, t_gt = (torch.as_tensor(d[k], device=dev) for k in ("pts_3d", "K", "R_gt", "t_gt"))
for it in range(31):
    R, t, status = pnp_batch_diff(x, X, K, certified_only=False)
    loss = ((R - R_gt) ** 2).sum((1, 2)) + ((t - t_gt) ** 2).sum(1)
    if it % 10 == 0:
        print(f"step {it:2d}: mean pose error {loss.detach().sqrt().mean().item():.3e}, certified {(status == 0).float().mean().item():.3f}")
    if it == 0:
        first = loss.detach().sqrt().mean().item()
    if it == 30:
        break
    x.grad = None
    loss.sum().backward()
    with torch.no_grad():
        x -= (0.5 * loss.detach() / (x.grad ** 2).sum((1, 2)).clamp_min(1e-300))[:, None, None] * x.grad
last = loss.detach().sqrt().mean().item()
assert last < 0.1 * first, (first, last)
print(f"pose error {first:.3e} -> {last:.3e}")
