"""Frames per second of ransac_pnpl_batch(confidence=..., local_opt=n) against the call without local optimisation, in one process.

    python tools/ransac_pnpl_lo_rate.py [--out DIR] [--quick] [--parent-module PATH]

1024 frames of 100 points + 50 lines (1 px noise) under a cap of 1024 hypotheses with confidence=0.99 in rounds of 64, for three frame
sets at thresh 2: 30 % clutter, 50 % clutter, and a mixed set whose clutter runs from 0 to 60 % over the frames (among points and among
lines alike).  Four calls per set -- "parent" (the call without the keywords; with --parent-module PATH, cvxpnpl_amd/ransac.py of another
checkout whose libraries are built: the parent commit's own call), "lo0" (local_opt=0), "lo1" (local_opt=1, lo_widen=2) and "lo3"
(local_opt=3, lo_widen=2) -- on scenes that are on the device before the clock starts.  Every timed call ends in its read-back, each set is
warmed up once, the calls are timed in alternation, and medians are reported with the spread (min .. max) of the repeats, by a host clock
around the call and by device events; the summed hyp_used and the rounds stand beside each.  Every active scene is refitted in every
round, changed or not (no skip list): that cost is inside the figures.

One JSON line per record; with --out also DIR/pnpl_lo_rate.jsonl."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, L, F, CAP, CONF, ROUND, THRESH = 100, 50, 1024, 1024, 0.99, 64, 2.0
SETS = (("clutter_30", lambda f, n: 0.3, THRESH), ("clutter_50", lambda f, n: 0.5, THRESH), ("mixed_0_60", lambda f, n: 0.6 * f / (n - 1), THRESH))


def frames(share, n=F, seed0=100):
    import numpy as np

    from cvxpnpl_amd import synth

    ds = [synth.make_ransac_pnpl(n_pts=P, n_lines=L, outlier_frac=share(f, n), sigma=1.0, seed=seed0 + f) for f in range(n)]
    return tuple(np.concatenate([d[k] for d in ds]) for k in ("pts_2d", "line_2d", "pts_3d", "line_3d"))


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


def rate_set(name, share, thresh, reps, parent_fn, n_frames):
    import torch

    from cvxpnpl_amd import ransac, synth

    dev = torch.device("cuda:0")
    args = tuple(torch.as_tensor(a, device=dev) for a in frames(share, n_frames)) + (torch.as_tensor(synth.K_KINECT, device=dev),)
    kw = dict(n_hyp=CAP, thresh=thresh, seed=0, sizes=[P] * n_frames, line_sizes=[L] * n_frames, device=dev, confidence=CONF, round_hyp=ROUND)
    calls = {"parent": lambda: parent_fn(*args, **kw), "lo0": lambda: ransac.ransac_pnpl_batch(*args, local_opt=0, **kw),
             "lo1": lambda: ransac.ransac_pnpl_batch(*args, local_opt=1, lo_widen=2.0, **kw),
             "lo3": lambda: ransac.ransac_pnpl_batch(*args, local_opt=3, lo_widen=2.0, **kw)}
    outs = {k: fn() for k, fn in calls.items()}   # warm-up of everything at this shape
    times = {k: [] for k in calls}
    for _ in range(reps):   # alternating
        for k, fn in calls.items():
            times[k].append(timed(fn))
    same = ("R", "t", "inliers_pts", "inliers_lines", "head", "hyp_used")
    rec = {"leg": "rate", "set": name, "F": n_frames, "cap": CAP, "confidence": CONF, "round_hyp": ROUND, "P": P, "L": L, "thresh": thresh, "reps": reps,
           "lo0_equals_parent": all(bool(torch.equal(outs["lo0"][k], outs["parent"][k])) for k in same),
           "no_scene_draws_more": all(bool((outs[k]["hyp_used"] <= outs["parent"]["hyp_used"]).all()) for k in ("lo1", "lo3"))}
    for k, v in times.items():
        rec[k] = {"fps_wall": round(n_frames / _med(v, 1), 1), "fps_events": round(n_frames / _med(v, 0), 1),
                  "ms_min_med_max": [round(min(t[1] for t in v) * 1e3, 3), round(_med(v, 1) * 1e3, 3), round(max(t[1] for t in v) * 1e3, 3)],
                  "hyp": int(outs[k]["hyp_used"].sum()), "rounds": outs[k]["rounds"], "mean_inliers": round(float(outs[k]["n_inliers"].double().mean()), 2)}
        if "lo_taken" in outs[k]:
            rec[k]["refits_taken"] = int(outs[k]["lo_taken"].sum())
    for k in ("lo0", "lo1", "lo3"):
        rec[k + "_over_parent_wall"] = round(_med(times[k], 1) / _med(times["parent"], 1), 4)
    lo, hi = min(t[1] for t in times["parent"]), max(t[1] for t in times["parent"])
    rec["lo0_inside_parent_spread"] = bool(lo <= _med(times["lo0"], 1) <= hi)
    print(json.dumps(rec), flush=True)
    return rec


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repeats and 256 frames")
    ap.add_argument("--parent-module", default=None, help="cvxpnpl_amd/ransac.py of another checkout: the call of the parent commit")
    a = ap.parse_args(argv)
    import torch

    from cvxpnpl_amd import ransac

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    parent_fn = ransac.ransac_pnpl_batch
    if a.parent_module:   # the parent's package under another name, beside this one
        pkg = os.path.dirname(os.path.abspath(a.parent_module))
        spec = importlib.util.spec_from_file_location("cvxpnpl_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["cvxpnpl_amd_parent"] = mod
        spec.loader.exec_module(mod)
        parent_fn = mod.ransac.ransac_pnpl_batch
    recs = [rate_set(name, share, thresh, reps=3 if a.quick else 9, parent_fn=parent_fn, n_frames=256 if a.quick else F) for name, share, thresh in SETS]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "pnpl_lo_rate.jsonl"), "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
