"""Cost of the pose backward (cvxpnpl_pose_vjp_batch) against the forward solve, timed with device events.

    python tools/grad_rate.py [--reps 20] [--out FILE]

Per shape: the forward (pnp_batch) alone, forward + backward through pnp_batch_diff (gradients for pts_2d and pts_3d), and the
VJP launch(es) alone (pose_vjp at the forward's poses).  Bytes are algorithmic: per point 40 B read for the reduction, and 40 B
read + 40 B written for the scatter (the large-N path reads the records twice; the 16-lane path keeps them in cache), plus the
per-problem pose, status, camera and upstream gradients; the rate is held against 8 TB/s.  One JSON line per shape.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, synth  # noqa: E402
from cvxpnpl_amd.grad import pnp_batch_diff, pose_vjp  # noqa: E402

SHAPES = [(10_000, 10), (125_000, 10), (16, 10_000)]
HBM = 8.0e12


def _time(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    for batch, n in SHAPES:
        d = synth.make_pnp(batch, n, sigma=1.0, seed=5)
        p2, p3, K = (torch.as_tensor(d[k], device=dev) for k in ("pts_2d", "pts_3d", "K"))
        gR, gt = torch.randn(batch, 3, 3, device=dev, dtype=torch.float64), torch.randn(batch, 3, device=dev, dtype=torch.float64)
        fwd = _time(lambda: pnp_batch(p2, p3, K), a.reps)

        def both():
            q2, q3 = p2.clone().requires_grad_(), p3.clone().requires_grad_()
            R, t, _ = pnp_batch_diff(q2, q3, K)
            ((R * gR).sum() + (t * gt).sum()).backward()

        fb = _time(both, a.reps)
        res = pnp_batch(p2, p3, K)
        bwd = _time(lambda: pose_vjp(res.R, res.t, res.status, gR, gt, pts_2d=p2, pts_3d=p3, K=K), a.reps)
        large = n >= 768
        per_point = (40 + 40 + 40) if large else (40 + 40)
        nbytes = batch * n * per_point + batch * (9 + 3 + 9 + 3) * 8 + batch * 4 * 2
        rec = {"batch": batch, "n": n, "forward_us": round(fwd, 1), "forward_backward_us": round(fb, 1), "vjp_us": round(bwd, 1),
               "vjp_share_of_forward": round(bwd / fwd, 4), "path": "multi-block" if large else "16-lane", "bytes": nbytes,
               "gb_per_s": round(nbytes / (bwd * 1e-6) / 1e9, 1), "fraction_of_8TBps": round(nbytes / (bwd * 1e-6) / HBM, 4)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
