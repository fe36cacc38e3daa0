"""Cost of the reprojection refinement (cvxpnpl_refine_batch / cvxpnpl_refine_scenes) beside the solves it follows, timed with device
events.

    python tools/refine_rate.py [--reps 20] [--out FILE]

- batch: 10 k problems of N = 10 at sigma = 1 px, started from pnp_batch's poses: the forward solve, the refinement launch, the
  refinement with covariance (a second launch), and the mean number of trials.
- scenes: 256 scenes of 100 points + 50 lines with 30 % outliers at sigma = 1 px, started from the RANSAC consensus: the RANSAC call
  without and with polish, and the refine_scenes launch alone on the consensus masks.
One JSON line per workload.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, ransac, refine, synth  # noqa: E402


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

    batch, n = 10_000, 10
    d = synth.make_pnp(batch, n, sigma=1.0, seed=5)
    p2, p3, K = (torch.as_tensor(d[k], device=dev) for k in ("pts_2d", "pts_3d", "K"))
    fwd = _time(lambda: pnp_batch(p2, p3, K), a.reps)
    sol = pnp_batch(p2, p3, K)
    kw = dict(pts_2d=p2, pts_3d=p3, K=K, status=sol.status)
    ref_us = _time(lambda: refine.refine_pose_batch(sol.R, sol.t, **kw), a.reps)
    cov_us = _time(lambda: refine.refine_pose_batch(sol.R, sol.t, want_cov=True, **kw), a.reps)
    res = refine.refine_pose_batch(sol.R, sol.t, **kw)
    done = res.status <= 1
    rec = {"workload": "batch", "batch": batch, "n": n, "forward_us": round(fwd, 1), "refine_us": round(ref_us, 1), "refine_with_cov_us": round(cov_us, 1),
           "refine_share_of_forward": round(ref_us / fwd, 4), "refined": int(done.sum()), "converged": int((res.status == 0).sum()),
           "mean_trials": round(float(res.iters[done].double().mean()), 2),
           "rms_px_before": round(float(torch.sqrt(res.cost[done, 0] / (2 * n)).mean()), 4), "rms_px_after": round(float(torch.sqrt(res.cost[done, 1] / (2 * n)).mean()), 4)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    F = 256
    ds = [synth.make_ransac_pnpl(100, 50, outlier_frac=0.3, sigma=1.0, seed=400 + f) for f in range(F)]
    args = ([x["pts_2d"] for x in ds], [x["line_2d"] for x in ds], [x["pts_3d"] for x in ds], [x["line_3d"] for x in ds], synth.K_KINECT)
    rkw = dict(n_hyp=256, seed=1, device=dev)
    plain_us = _time(lambda: ransac.ransac_pnpl_batch(*args, **rkw), max(3, a.reps // 4))
    polish_us = _time(lambda: ransac.ransac_pnpl_batch(*args, polish=True, **rkw), max(3, a.reps // 4))
    out = ransac.ransac_pnpl_batch(*args, **rkw)
    sc = ransac.pack_pnpl_scenes(*args, device=dev)
    mp, ml = out["inliers_pts"].view(torch.uint8), out["inliers_lines"].view(torch.uint8)
    sc_us = _time(lambda: refine.refine_scenes(sc, out["R"], out["t"], mask_pts=mp, mask_lines=ml), a.reps)
    res = refine.refine_scenes(sc, out["R"], out["t"], mask_pts=mp, mask_lines=ml)
    done = res.status <= 1
    rec = {"workload": "scenes", "scenes": F, "points": 100, "lines": 50, "ransac_us": round(plain_us, 1), "ransac_polish_us": round(polish_us, 1),
           "refine_scenes_us": round(sc_us, 1), "refined": int(done.sum()), "converged": int((res.status == 0).sum()),
           "mean_trials": round(float(res.iters[done].double().mean()), 2), "mean_live": round(float(res.n_live.double().mean()), 1)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
