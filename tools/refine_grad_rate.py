"""Cost of the refinement's backward pass (cvxpnpl_refine_vjp_batch / cvxpnpl_refine_vjp_scenes) beside the forward refinement of the same
inputs in the same run, timed with device events (median of --reps).

    python tools/refine_grad_rate.py [--reps 20] [--out FILE]

- batch: 10 k problems of N = 10 at sigma = 1 px, refined from pnp_batch's poses: the refine_pose_batch launch and the refine_vjp launch
  at its poses.
- scenes: 256 scenes of 100 points + 50 lines at sigma = 1 px, refined from the ground truth: the refine_scenes launch and the
  refine_vjp_scenes launch at its poses.
One JSON line per workload.  No rate is promised: the figures are what DESIGN.md section 16 records.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, ransac, refine, refine_grad, synth  # noqa: E402


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
    sol = pnp_batch(p2, p3, K)
    kw = dict(pts_2d=p2, pts_3d=p3, K=K)
    fwd_us = _time(lambda: refine.refine_pose_batch(sol.R, sol.t, status=sol.status, **kw), a.reps)
    res = refine.refine_pose_batch(sol.R, sol.t, status=sol.status, **kw)
    gR, gt = torch.randn_like(res.R), torch.randn_like(res.t)
    vjp_us = _time(lambda: refine_grad.refine_vjp(res.R, res.t, res.status, gR, gt, **kw), a.reps)
    out = refine_grad.refine_vjp(res.R, res.t, res.status, gR, gt, want_info=True, **kw)
    ok = out["vjp_status"] == 0
    rec = {"workload": "batch", "batch": batch, "n": n, "refine_us": round(fwd_us, 1), "refine_vjp_us": round(vjp_us, 1),
           "vjp_share_of_refine": round(vjp_us / fwd_us, 4), "converged": int((res.status == 0).sum()), "differentiated": int(ok.sum()),
           "max_stationarity": float(out["info"][ok, 0].max()), "min_pivot_ratio": float(out["info"][ok, 1].min())}
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    F = 256
    ds = [synth.make_pnpl(1, 100, 50, sigma=1.0, seed=400 + f) for f in range(F)]
    sc = ransac.pack_pnpl_scenes([x["pts_2d"][0] for x in ds], [x["line_2d"][0] for x in ds], [x["pts_3d"][0] for x in ds],
                                 [x["line_3d"][0] for x in ds], synth.K_KINECT, device=dev)
    R0 = torch.as_tensor(np.concatenate([x["R_gt"] for x in ds]), device=dev)
    t0 = torch.as_tensor(np.concatenate([x["t_gt"] for x in ds]) * 1.01, device=dev)
    fwd_us = _time(lambda: refine.refine_scenes(sc, R0, t0), a.reps)
    res = refine.refine_scenes(sc, R0, t0)
    gR, gt = torch.randn_like(res.R), torch.randn_like(res.t)
    vjp_us = _time(lambda: refine_grad.refine_vjp_scenes(sc, res.R, res.t, res.status, gR, gt), a.reps)
    out = refine_grad.refine_vjp_scenes(sc, res.R, res.t, res.status, gR, gt)
    rec = {"workload": "scenes", "scenes": F, "points": 100, "lines": 50, "refine_scenes_us": round(fwd_us, 1), "refine_vjp_scenes_us": round(vjp_us, 1),
           "vjp_share_of_refine": round(vjp_us / fwd_us, 4), "converged": int((res.status == 0).sum()),
           "differentiated": int((out["vjp_status"] == 0).sum())}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
