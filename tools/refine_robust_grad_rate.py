"""Cost of the robust refinement's backward pass (cvxpnpl_refine_robust_vjp_batch / cvxpnpl_refine_robust_vjp_scenes) beside the robust
forward of the same inputs and the least-squares backward pass (refine_vjp) on the same inputs, in the same run, timed with device
events (median of --reps).

    python tools/refine_robust_grad_rate.py [--reps 20] [--out FILE]

- batch: 10 k problems of N = 10 at sigma = 1 px, refined from pnp_batch's poses under each loss (delta = 2 px), weights uniform in
  [0.25, 4]: the refine_pose_batch_robust launches, the refine_vjp_robust launch at its poses, and refine_vjp at the same poses.
- scenes: 256 scenes of 100 points + 50 lines at sigma = 1 px, refined from the ground truth: refine_scenes_robust, the
  refine_vjp_scenes_robust launch at its poses, and refine_vjp_scenes at the same poses.
One JSON line per workload and loss.  No rate is promised: the figures are what DESIGN.md section 18 records.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, ransac, refine_grad, refine_robust, refine_robust_grad, synth  # noqa: E402

ADMIT = 0x3  # converged and max_iters: the robust forward leaves some problems at max_iters


def _time(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ts.append(start.elapsed_time(stop) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _summary(out, status):
    ok = out["vjp_status"] == 0
    return {"converged": int((status == 0).sum()), "differentiated": int(ok.sum()), "share_differentiated": round(float(ok.double().mean()), 4),
            "max_stationarity": float(out["info"][ok, 0].max()), "min_pivot_ratio": float(out["info"][ok, 1].min())}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lines = []

    batch, n = 10_000, 10
    d = synth.make_pnp(batch, n, sigma=1.0, seed=5)
    p2, p3, K = (torch.as_tensor(d[k], device=dev) for k in ("pts_2d", "pts_3d", "K"))
    w = torch.as_tensor(np.random.RandomState(6).uniform(0.25, 4.0, (batch, n)), device=dev)
    sol = pnp_batch(p2, p3, K)
    kw = dict(pts_2d=p2, pts_3d=p3, K=K)
    for loss in ("l2", "huber", "cauchy"):
        rk = dict(loss=loss, scale_px=2.0, weights_pts=w)
        fwd_us = _time(lambda: refine_robust.refine_pose_batch_robust(sol.R, sol.t, status=sol.status, **kw, **rk), a.reps)
        res = refine_robust.refine_pose_batch_robust(sol.R, sol.t, status=sol.status, **kw, **rk)
        gR, gt = torch.randn_like(res.R), torch.randn_like(res.t)
        vjp_us = _time(lambda: refine_robust_grad.refine_vjp_robust(res.R, res.t, res.status, gR, gt, admit_mask=ADMIT, **kw, **rk), a.reps)
        ls_us = _time(lambda: refine_grad.refine_vjp(res.R, res.t, res.status, gR, gt, admit_mask=ADMIT, **kw), a.reps)
        out = refine_robust_grad.refine_vjp_robust(res.R, res.t, res.status, gR, gt, admit_mask=ADMIT, want_info=True, **kw, **rk)
        rec = {"workload": "batch", "loss": loss, "batch": batch, "n": n, "refine_robust_us": round(fwd_us, 1), "refine_vjp_robust_us": round(vjp_us, 1),
               "refine_vjp_us": round(ls_us, 1), "robust_vjp_over_vjp": round(vjp_us / ls_us, 4), "vjp_share_of_forward": round(vjp_us / fwd_us, 4)}
        rec.update(_summary(out, res.status))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    F = 256
    ds = [synth.make_pnpl(1, 100, 50, sigma=1.0, seed=400 + f) for f in range(F)]
    sc = ransac.pack_pnpl_scenes([x["pts_2d"][0] for x in ds], [x["line_2d"][0] for x in ds], [x["pts_3d"][0] for x in ds],
                                 [x["line_3d"][0] for x in ds], synth.K_KINECT, device=dev)
    R0 = torch.as_tensor(np.concatenate([x["R_gt"] for x in ds]), device=dev)
    t0 = torch.as_tensor(np.concatenate([x["t_gt"] for x in ds]) * 1.01, device=dev)
    rs = np.random.RandomState(7)
    wp, wl = torch.as_tensor(rs.uniform(0.25, 4.0, F * 100), device=dev), torch.as_tensor(rs.uniform(0.25, 4.0, F * 50), device=dev)
    for loss in ("l2", "huber", "cauchy"):
        rk = dict(loss=loss, scale_px=2.0, weights_pts=wp, weights_lines=wl)
        fwd_us = _time(lambda: refine_robust.refine_scenes_robust(sc, R0, t0, **rk), a.reps)
        res = refine_robust.refine_scenes_robust(sc, R0, t0, **rk)
        gR, gt = torch.randn_like(res.R), torch.randn_like(res.t)
        vjp_us = _time(lambda: refine_robust_grad.refine_vjp_scenes_robust(sc, res.R, res.t, res.status, gR, gt, admit_mask=ADMIT, **rk), a.reps)
        ls_us = _time(lambda: refine_grad.refine_vjp_scenes(sc, res.R, res.t, res.status, gR, gt, admit_mask=ADMIT), a.reps)
        out = refine_robust_grad.refine_vjp_scenes_robust(sc, res.R, res.t, res.status, gR, gt, admit_mask=ADMIT, want_info=True, **rk)
        rec = {"workload": "scenes", "loss": loss, "scenes": F, "points": 100, "lines": 50, "refine_scenes_robust_us": round(fwd_us, 1),
               "refine_vjp_scenes_robust_us": round(vjp_us, 1), "refine_vjp_scenes_us": round(ls_us, 1), "robust_vjp_over_vjp": round(vjp_us / ls_us, 4),
               "vjp_share_of_forward": round(vjp_us / fwd_us, 4)}
        rec.update(_summary(out, res.status))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
