"""Frames per second of ransac_pnp_batch(scoring="msac") against scoring="count", and the pose error of the two winners, in one process.

    python tools/ransac_msac_rate.py [--out DIR] [--quick] [--parent-module PATH]

Rate: 256 frames x 256 hypotheses (fixed budget), and 1024 frames under a cap of 1024 with confidence=0.99 in rounds of 64; frames of 100
correspondences, 30 % clutter, 1 px noise, thresh 4.  Three calls per shape -- "parent" (the call without the keyword; with
--parent-module PATH, cvxpnpl_amd/ransac.py of another checkout whose libraries are built: the parent commit's own count call), "count"
(scoring="count") and "msac" -- on scenes that are on the device before the clock starts.  Every timed call ends in its read-back, each
shape is warmed up once, the calls are timed in alternation, and medians are reported with the spread (min .. max) of the repeats, by a
host clock around the call and by device events.

Pose error: the rotation error of the selected minimal hypothesis (refit=False, seed=0) against the ground truth over 48 frames, count
winner against MSAC winner among the same draws, at the settings of DESIGN.md section 23.

One JSON line per record; with --out also DIR/msac_rate.jsonl."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 100
RATE_SHAPES = ((256, 256, None), (1024, 1024, 0.99))   # frames, n_hyp (the cap with a confidence), confidence
POSE_SETTINGS = (dict(thresh=4.0, n_hyp=128, outlier_frac=0.3, sigma=1.0), dict(thresh=2.0, n_hyp=128, outlier_frac=0.3, sigma=1.0),
                 dict(thresh=6.0, n_hyp=64, outlier_frac=0.3, sigma=1.0), dict(thresh=2.0, n_hyp=256, outlier_frac=0.5, sigma=0.5))


def frames(F, outlier_frac=0.3, sigma=1.0, seed0=100):
    import numpy as np

    from cvxpnpl_amd import synth

    ds = [synth.make_ransac(1, n_corr=M, outlier_frac=outlier_frac, sigma=sigma, seed=seed0 + f) for f in range(F)]
    return np.concatenate([d["scene_2d"] for d in ds]), np.concatenate([d["scene_3d"] for d in ds]), np.stack([d["R_gt"] for d in ds])


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, time.perf_counter() - w, out


def _med(v, k):
    return sorted(t[k] for t in v)[len(v) // 2]


def rate_shape(F, n_hyp, conf, reps, parent_fn):
    import torch

    from cvxpnpl_amd import ransac, synth

    dev = torch.device("cuda:0")
    x, X, _ = frames(F)
    x, X, K = torch.as_tensor(x, device=dev), torch.as_tensor(X, device=dev), torch.as_tensor(synth.K_KINECT, device=dev)
    kw = dict(n_hyp=n_hyp, thresh=4.0, seed=0, sizes=[M] * F, device=dev)
    if conf is not None:
        kw.update(confidence=conf, round_hyp=64)
    calls = {"parent": lambda: parent_fn(x, X, K, **kw), "count": lambda: ransac.ransac_pnp_batch(x, X, K, scoring="count", **kw),
             "msac": lambda: ransac.ransac_pnp_batch(x, X, K, scoring="msac", **kw)}
    outs = {k: fn() for k, fn in calls.items()}   # warm-up of everything at this shape
    times = {k: [] for k in calls}
    for _ in range(reps):   # alternating
        for k, fn in calls.items():
            times[k].append(timed(fn))
    rec = {"leg": "rate", "F": F, "n_hyp": n_hyp, "confidence": conf, "M": M, "reps": reps,
           "count_equals_parent": all(bool(torch.equal(outs["count"][k], outs["parent"][k])) for k in ("R", "t", "inliers", "head"))}
    for k, v in times.items():
        rec[k] = {"fps_wall": round(F / _med(v, 1), 1), "fps_events": round(F / _med(v, 0), 1),
                  "ms_min_med_max": [round(min(t[1] for t in v) * 1e3, 3), round(_med(v, 1) * 1e3, 3), round(max(t[1] for t in v) * 1e3, 3)]}
        if conf is not None:
            rec[k].update(hyp=int(outs[k]["hyp_used"].sum()), rounds=outs[k]["rounds"])
    rec["msac_over_count_wall"] = round(_med(times["msac"], 1) / _med(times["count"], 1), 4)
    rec["msac_over_parent_wall"] = round(_med(times["msac"], 1) / _med(times["parent"], 1), 4)
    rec["count_over_parent_wall"] = round(_med(times["count"], 1) / _med(times["parent"], 1), 4)
    print(json.dumps(rec), flush=True)
    return rec


def pose_error(thresh, n_hyp, outlier_frac, sigma, F=48):
    import numpy as np
    import torch

    from cvxpnpl_amd import ransac, synth

    dev = torch.device("cuda:0")
    x, X, R_gt = frames(F, outlier_frac, sigma)
    kw = dict(n_hyp=n_hyp, thresh=thresh, seed=0, refit=False, sizes=[M] * F, device=dev)
    err, count = {}, None
    for scoring in ("count", "msac"):
        out = ransac.ransac_pnp_batch(x, X, synth.K_KINECT, scoring=scoring, **kw)
        err[scoring] = np.degrees(synth.geodesic(out["R"].cpu().numpy(), R_gt))
        if scoring == "count":   # scenes where the highest count is shared: the hypotheses scored again, as the call scored them
            sc = ransac.pack_scenes(x, X, synth.K_KINECT, sizes=[M] * F, device=dev, seeds=list(range(F)))
            p2, p3, _ = ransac.sample_scenes(sc, n_hyp)
            res = ransac.pnp_batch(p2, p3, sc.K, eps=1e-6, max_iters=100, device=dev)
            count = ransac.score_scenes(sc, res.R, res.t, thresh, status=res.status).cpu().numpy().reshape(F, n_hyp)
    c, m = err["count"], err["msac"]
    rec = {"leg": "pose_error", "F": F, "M": M, "thresh": thresh, "n_hyp": n_hyp, "outlier_frac": outlier_frac, "sigma": sigma,
           "count_mean_deg": round(float(c.mean()), 4), "count_median_deg": round(float(np.median(c)), 4),
           "msac_mean_deg": round(float(m.mean()), 4), "msac_median_deg": round(float(np.median(m)), 4),
           "ratio_of_means": round(float(m.mean() / c.mean()), 3), "scenes_tied_on_count": int(((count == count.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum()),
           "msac_better": int((m < c).sum()), "equal": int((m == c).sum()), "msac_worse": int((m > c).sum())}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    ap.add_argument("--parent-module", default=None, help="cvxpnpl_amd/ransac.py of another checkout: the count call of the parent commit")
    a = ap.parse_args(argv)
    import torch

    from cvxpnpl_amd import ransac

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    parent_fn = ransac.ransac_pnp_batch
    if a.parent_module:   # the parent's package under another name, beside this one
        pkg = os.path.dirname(os.path.abspath(a.parent_module))
        spec = importlib.util.spec_from_file_location("cvxpnpl_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["cvxpnpl_amd_parent"] = mod
        spec.loader.exec_module(mod)
        parent_fn = mod.ransac.ransac_pnp_batch
    recs = [pose_error(**s) for s in POSE_SETTINGS]
    for F, n_hyp, conf in RATE_SHAPES:
        recs.append(rate_shape(F, n_hyp, conf, reps=(5 if a.quick else 15) if F <= 256 else (3 if a.quick else 9), parent_fn=parent_fn))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "msac_rate.jsonl"), "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
