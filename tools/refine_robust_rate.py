"""Cost of the robust reprojection refinement (cvxpnpl_refine_robust_batch / cvxpnpl_refine_robust_scenes) beside the least-squares
refinement on the same inputs in the same run, timed with device events (median of --reps, the two alternating).

    python tools/refine_robust_rate.py [--reps 20] [--out FILE]

- batch: 10 k problems of N = 10 at sigma = 1 px, started from pnp_batch's poses: refine_pose_batch, then refine_pose_batch_robust under
  each loss (delta = 2 px), with the mean number of trials and the rms pixel error of the records before and after.
- scenes: 256 scenes of 100 points + 50 lines with 30 % outliers at sigma = 1 px, started from the RANSAC poses: refine_scenes over the
  consensus masks, and refine_scenes_robust (Huber, delta = the RANSAC threshold) over ALL records with no mask; the rms pixel error of
  the TRUE inliers (those the generator did not displace) at the pose before and after each.
One JSON line per workload.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvxpnpl_amd import pnp_batch, ransac, refine, refine_robust, synth  # noqa: E402


def _time_pair(fns, reps):
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


def _rms_true_inliers(ds, R, t):
    """rms pixel error over the scenes' true inlier points and line end points at the poses (R, t) [F]."""
    R, t = R.cpu().numpy(), t.cpu().numpy()
    sq, cnt = 0.0, 0
    for f, d in enumerate(ds):
        K = d["K"]
        X, x = d["pts_3d"][d["inlier_pts"]], d["pts_2d"][d["inlier_pts"]]
        h = (X @ R[f].T + t[f]) @ K.T
        sq += float((((h[:, :2] / h[:, 2:]) - x) ** 2).sum())
        cnt += 2 * len(X)
        l2, l3 = d["line_2d"][d["inlier_lines"]], d["line_3d"][d["inlier_lines"]]
        a, b = np.concatenate([l2[:, 0], np.ones((len(l2), 1))], 1), np.concatenate([l2[:, 1], np.ones((len(l2), 1))], 1)
        ln = np.cross(a, b)
        ln /= np.hypot(ln[:, 0], ln[:, 1])[:, None]
        for e in (0, 1):
            h = (l3[:, e] @ R[f].T + t[f]) @ K.T
            sq += float(((ln[:, 0] * h[:, 0] / h[:, 2] + ln[:, 1] * h[:, 1] / h[:, 2] + ln[:, 2]) ** 2).sum())
            cnt += len(l2)
    return (sq / cnt) ** 0.5


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/refine_robust_rate.py measures on a GPU and none is visible")
    dev = torch.device("cuda:0")
    lines = []

    batch, n, delta = 10_000, 10, 2.0
    d = synth.make_pnp(batch, n, sigma=1.0, seed=5)
    p2, p3, K = (torch.as_tensor(d[k], device=dev) for k in ("pts_2d", "pts_3d", "K"))
    sol = pnp_batch(p2, p3, K)
    kw = dict(pts_2d=p2, pts_3d=p3, K=K, status=sol.status)
    fns = [lambda: refine.refine_pose_batch(sol.R, sol.t, **kw)]
    fns += [lambda loss=loss: refine_robust.refine_pose_batch_robust(sol.R, sol.t, loss=loss, scale_px=delta, **kw) for loss in refine_robust.LOSSES]
    times = _time_pair(fns, a.reps)
    rec = {"workload": "batch", "batch": batch, "n": n, "delta_px": delta, "refine_us": round(times[0], 1)}
    base = refine.refine_pose_batch(sol.R, sol.t, **kw)
    done = base.status <= 1
    rec["refine_mean_trials"] = round(float(base.iters[done].double().mean()), 2)
    rec["refine_max_trials"] = int(base.iters.max())
    rec["rms_px_before"] = round(float(torch.sqrt(base.cost[done, 0] / (2 * n)).mean()), 4)
    rec["refine_rms_px_after"] = round(float(torch.sqrt(base.cost[done, 1] / (2 * n)).mean()), 4)
    for loss, us in zip(refine_robust.LOSSES, times[1:]):
        res = refine_robust.refine_pose_batch_robust(sol.R, sol.t, loss=loss, scale_px=delta, **kw)
        ok = res.status <= 1
        # the rms pixel error of ALL records at the returned pose: the least-squares cost there, from a zero-trial least-squares call
        at = refine.refine_pose_batch(res.R, res.t, max_iters=0, **kw)
        rec[loss] = {"us": round(us, 1), "ratio_to_refine": round(us / times[0], 3), "refined": int(ok.sum()), "converged": int((res.status == 0).sum()),
                     "mean_trials": round(float(res.iters[ok].double().mean()), 2), "max_trials": int(res.iters.max()), "rms_px_after": round(float(torch.sqrt(at.cost[ok, 0] / (2 * n)).mean()), 4),
                     "mean_inliers": round(float(res.n_inlier[ok].double().mean()), 2)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    F, thresh = 256, 2.0
    ds = [synth.make_ransac_pnpl(100, 50, outlier_frac=0.3, sigma=1.0, seed=400 + f) for f in range(F)]
    args = ([x["pts_2d"] for x in ds], [x["line_2d"] for x in ds], [x["pts_3d"] for x in ds], [x["line_3d"] for x in ds], synth.K_KINECT)
    out = ransac.ransac_pnpl_batch(*args, n_hyp=256, thresh=thresh, seed=1, device=dev)
    sc = ransac.pack_pnpl_scenes(*args, device=dev)
    mp, ml = out["inliers_pts"].view(torch.uint8), out["inliers_lines"].view(torch.uint8)
    head = out["head"].to(dev)
    masked = lambda: refine.refine_scenes(sc, out["R"], out["t"], mask_pts=mp, mask_lines=ml, status=head[:, 0])  # noqa: E731
    robust = lambda: refine_robust.refine_scenes_robust(sc, out["R"], out["t"], loss="huber", scale_px=thresh, status=head[:, 0])  # noqa: E731
    t_masked, t_robust = _time_pair([masked, robust], a.reps)
    m, r = masked(), robust()
    rec = {"workload": "scenes", "scenes": F, "points": 100, "lines": 50, "outlier_frac": 0.3, "delta_px": thresh,
           "refine_scenes_masked_us": round(t_masked, 1), "refine_scenes_robust_us": round(t_robust, 1), "ratio": round(t_robust / t_masked, 3),
           "masked_mean_trials": round(float(m.iters[m.status <= 1].double().mean()), 2), "robust_mean_trials": round(float(r.iters[r.status <= 1].double().mean()), 2),
           "masked_max_trials": int(m.iters.max()), "robust_max_trials": int(r.iters.max()), "masked_converged": int((m.status == 0).sum()), "robust_converged": int((r.status == 0).sum()),
           "masked_mean_live": round(float(m.n_live.double().mean()), 1), "robust_mean_live": round(float(r.n_live.double().mean()), 1),
           "robust_mean_inliers": round(float(r.n_inlier.double().mean()), 1),
           "rms_px_true_inliers_before": round(_rms_true_inliers(ds, out["R"], out["t"]), 4),
           "rms_px_true_inliers_masked": round(_rms_true_inliers(ds, m.R, m.t), 4), "rms_px_true_inliers_robust": round(_rms_true_inliers(ds, r.R, r.t), 4)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
