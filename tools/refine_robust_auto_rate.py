"""Cost of the robust refinement at an estimated scale per problem (cvxpnpl_amd.refine_robust_auto) beside the seventh library's call at one
fixed scale on the same inputs in the same run, timed with device events (median of --reps, the functions alternating).

    python tools/refine_robust_auto_rate.py [--reps 20] [--out FILE]

- batch: 10 k problems of N = 10 at sigma = 1 px, started from pnp_batch's poses.
- scenes: 1024 scenes of 100 points + 50 lines with 30 % outliers at sigma = 1 px, started from the true pose moved by 0.01 rad and 1 %.
Per workload, Huber: refine_*_robust at scale 2 px (the baseline); the automatic call (one round: the scale kernel, then the loop at the
scale per problem) and the same with the covariance; the scale kernel alone; the covariance kernel alone at the poses reached.  Every
figure includes the Python wrapper's allocations and, for the automatic calls, the handful of element-wise launches that turn sigma into
a scale and merge the statuses.  One JSON line per workload.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, ransac, refine_robust, refine_robust_auto as ra, synth  # noqa: E402


def _time(fns, reps):
    """Median time in microseconds of each function, the functions taking turns inside every repetition."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ts[i].append(start.elapsed_time(stop) * 1e3)
    return [sorted(t)[len(t) // 2] for t in ts]


def _record(name, shape, times, fixed, auto):
    t_fixed, t_auto, t_auto_cov, t_scale, t_cov = times
    ok = auto.status <= 1
    return dict(workload=name, **shape, loss="huber", fixed_scale_px=2.0, fixed_us=round(t_fixed, 1), auto_us=round(t_auto, 1), auto_with_cov_us=round(t_auto_cov, 1),
                scale_kernel_us=round(t_scale, 1), cov_kernel_us=round(t_cov, 1), auto_over_fixed=round(t_auto / t_fixed, 3),
                scale_over_fixed=round(t_scale / t_fixed, 3), cov_over_fixed=round(t_cov / t_fixed, 3),
                fixed_mean_trials=round(float(fixed.iters[fixed.status <= 1].double().mean()), 2), auto_mean_trials=round(float(auto.iters[ok].double().mean()), 2),
                refined=int(ok.sum()), mean_sigma_px=round(float(auto.sigma_px[ok].mean()), 3), cov_ok=int(torch.isfinite(auto.cov[:, 0, 0]).sum()))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/refine_robust_auto_rate.py measures on a GPU and none is visible")
    dev = torch.device("cuda:0")
    lines = []

    batch, n = 10_000, 10
    d = synth.make_pnp(batch, n, sigma=1.0, seed=5)
    p2, p3, K = (torch.as_tensor(d[k], device=dev) for k in ("pts_2d", "pts_3d", "K"))
    sol = pnp_batch(p2, p3, K)
    kw = dict(pts_2d=p2, pts_3d=p3, K=K, status=sol.status)
    auto = ra.refine_pose_batch_robust_auto(sol.R, sol.t, loss="huber", covariance=True, **kw)
    fns = [lambda: refine_robust.refine_pose_batch_robust(sol.R, sol.t, loss="huber", scale_px=2.0, **kw),
           lambda: ra.refine_pose_batch_robust_auto(sol.R, sol.t, loss="huber", **kw),
           lambda: ra.refine_pose_batch_robust_auto(sol.R, sol.t, loss="huber", covariance=True, **kw),
           lambda: ra.robust_scale_batch(sol.R, sol.t, **kw),
           lambda: ra.robust_covariance_batch(auto.R, auto.t, pts_2d=p2, pts_3d=p3, K=K, loss="huber", scale_px=auto.scale_px, status=auto.status)]
    rec = _record("batch", dict(batch=batch, n=n), _time(fns, a.reps), fns[0](), auto)
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    F = 1024
    ds = [synth.make_ransac_pnpl(100, 50, outlier_frac=0.3, sigma=1.0, seed=400 + f) for f in range(F)]
    args = ([x["pts_2d"] for x in ds], [x["line_2d"] for x in ds], [x["pts_3d"] for x in ds], [x["line_3d"] for x in ds], synth.K_KINECT)
    sc = ransac.pack_pnpl_scenes(*args, device=dev)
    rs = np.random.RandomState(2)
    R0, t0 = [], []
    for x in ds:
        w = rs.normal(size=3)
        w *= 0.01 / np.linalg.norm(w)
        W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        R0.append((np.eye(3) + np.sin(0.01) / 0.01 * W + (1.0 - np.cos(0.01)) / 1e-4 * W @ W) @ x["R_gt"])
        t0.append(x["t_gt"] * (1.0 + 0.01 * rs.uniform(-1.0, 1.0, 3)))
    R0, t0 = torch.as_tensor(np.stack(R0), device=dev), torch.as_tensor(np.stack(t0), device=dev)
    auto = ra.refine_scenes_robust_auto(sc, R0, t0, loss="huber", covariance=True)
    fns = [lambda: refine_robust.refine_scenes_robust(sc, R0, t0, loss="huber", scale_px=2.0),
           lambda: ra.refine_scenes_robust_auto(sc, R0, t0, loss="huber"),
           lambda: ra.refine_scenes_robust_auto(sc, R0, t0, loss="huber", covariance=True),
           lambda: ra.robust_scale_scenes(sc, R0, t0),
           lambda: ra.robust_covariance_scenes(sc, auto.R, auto.t, loss="huber", scale_px=auto.scale_px, status=auto.status)]
    rec = _record("scenes", dict(scenes=F, points=100, lines=50, outlier_frac=0.3), _time(fns, a.reps), fns[0](), auto)
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
