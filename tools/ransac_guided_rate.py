"""Frames per second of ransac_pnp_batch(confidence=0.99, quality=...), the guided sampler, against the unguided adaptive call, in one process.

    python tools/ransac_guided_rate.py [--out DIR] [--quick] [--parent-module PATH]
    python tools/ransac_guided_rate.py --rank-trace DIR

Grid: F in {16, 256, 1024} scenes of M = 100 correspondences, every scene 50 % or 70 % clutter, cap 1024, confidence 0.99, round_hyp 64.
The method is that of tools/ransac_adaptive_rate.py: scenes and qualities are on the device before the clock starts, every timed call
ends in its read-back, each shape is warmed up once, the calls are timed in alternation, and medians are reported with the spread
(min .. max) of the repeats.  Timed per shape: the unguided adaptive call ("adaptive") and the fixed call with quality=None ("none") --
both through --parent-module PATH when given, cvxpnpl_amd/ransac.py of another checkout whose libraries are built, to time the parent
commit itself, and then "none" also through this package -- and the guided call with three qualities: "informative" (inliers U(0.2, 1),
clutter U(0, 0.8)), "constant" (all equal: the ranking is the identity) and "reversed" (the informative one negated: the cost of a bad
prior).  Per call: frames/s, hypotheses solved in all, rounds, and the share of poses within 1e-3 rad of the baseline's fixed call at the
cap.  One JSON line per shape; with --out also DIR/rate.jsonl.

--rank-trace DIR: the ranking kernel alone at M in {100, 1000, 10000} (256, 256 and 16 scenes).  The launches run in a child process of
its own under `rocprofv3 --kernel-trace`; the kernel's times are read from the trace and written to DIR/rank_kernel.jsonl.
"""
import argparse
import glob
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP, ROUND_HYP, CONF = 1024, 64, 0.99
RANK_SHAPES = ((256, 100), (256, 1000), (16, 10000))   # (scenes, correspondences per scene)
RANK_REPS = 5


def scenes(F, clutter, M=100, seed0=0):
    import numpy as np

    from cvxpnpl_amd import synth

    rs = np.random.RandomState(seed0 + 12345)
    xs, Xs, qs = [], [], []
    for f in range(F):
        d = synth.make_ransac(1, n_corr=M, outlier_frac=clutter, sigma=0.5, seed=seed0 + f)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"])
        qs.append(np.where(d["inlier"], rs.uniform(0.2, 1.0, M), rs.uniform(0.0, 0.8, M)))
    return xs, Xs, qs, synth.K_KINECT


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


def one_shape(F, clutter, reps, parent_fn):
    import numpy as np
    import torch

    from cvxpnpl_amd import ransac, synth

    dev = torch.device("cuda:0")
    xs, Xs, qs, K = scenes(F, clutter)
    xp = torch.cat([torch.as_tensor(a, device=dev) for a in xs])
    Xp = torch.cat([torch.as_tensor(a, device=dev) for a in Xs])
    q = torch.cat([torch.as_tensor(a, device=dev) for a in qs])
    Kd, sizes = torch.as_tensor(K, device=dev), [a.shape[0] for a in xs]
    base = parent_fn or ransac.ransac_pnp_batch
    kw = dict(n_hyp=CAP, seed=0, sizes=sizes, device=dev)
    qual = {"informative": q, "constant": torch.full_like(q, 0.5), "reversed": -q}
    calls = {"adaptive": lambda: base(xp, Xp, Kd, confidence=CONF, round_hyp=ROUND_HYP, **kw), "none": lambda: base(xp, Xp, Kd, **kw)}
    if parent_fn is not None:
        calls["none_here"] = lambda: ransac.ransac_pnp_batch(xp, Xp, Kd, quality=None, **kw)
    for name, qq in qual.items():
        calls[name] = (lambda qq: lambda: ransac.ransac_pnp_batch(xp, Xp, Kd, confidence=CONF, round_hyp=ROUND_HYP, quality=qq, **kw))(qq)
    ref = calls["none"]()   # the baseline's fixed call at the cap: the poses every other call is held against
    for fn in calls.values():   # warm-up of everything at this shape
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):   # alternating
        for name, fn in calls.items():
            times[name].append(timed(fn))
    Rf, nf = ref["R"].cpu().numpy(), ref["n_inliers"].numpy()
    ok = nf >= 4
    rec = {"F": F, "M": 100, "clutter": clutter, "cap": CAP, "round_hyp": ROUND_HYP, "confidence": CONF, "reps": reps,
           "baseline": "parent" if parent_fn is not None else "this package"}
    for name in calls:
        out, v = times[name][-1][2], times[name]
        r = {"fps_wall": round(F / _med(v, 1), 1), "fps_events": round(F / _med(v, 0), 1),
             "ms_min_max": [round(min(t[1] for t in v) * 1e3, 3), round(max(t[1] for t in v) * 1e3, 3)]}
        if "hyp_used" in out:
            r.update(hyp=int(out["hyp_used"].sum()), rounds=out["rounds"])
        else:
            r.update(hyp=F * CAP, rounds=1)
        if ok.any():
            geo = synth.geodesic(out["R"].cpu().numpy()[ok], Rf[ok])
            r["pose_within_1e-3_rad"] = round(float((geo < 1e-3).mean()), 4)
        rec[name] = r
    print(json.dumps(rec), flush=True)
    return rec


def rank_child():
    """The launches of --rank-trace: per shape one warm-up and RANK_REPS launches of the ranking, in the order of RANK_SHAPES."""
    import numpy as np
    import torch

    from cvxpnpl_amd import ransac

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    for F, M in RANK_SHAPES:
        sc = ransac.pack_scenes(rs.random_sample((F * M, 2)), rs.random_sample((F * M, 3)), np.eye(3), sizes=[M] * F, device=dev)
        q = torch.as_tensor(rs.random_sample(F * M), device=dev)
        for _ in range(1 + RANK_REPS):
            order = ransac.rank_scenes(sc, q)
        torch.cuda.synchronize()
        assert sorted(order[:M].tolist()) == list(range(M))


def rank_trace(out):
    import csv

    os.makedirs(out, exist_ok=True)
    tmp = os.path.join(out, "_rocprof_rank")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "rank", "--", sys.executable,
                        os.path.abspath(__file__), "--rank-child"], timeout=600)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not found:
        raise SystemExit(f"rocprofv3 run failed ({r.returncode})")
    rows = [row for f in found for row in csv.DictReader(open(f)) if "rank_quality_kernel" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    assert len(rows) == len(RANK_SHAPES) * (1 + RANK_REPS), len(rows)
    with open(os.path.join(out, "rank_kernel.jsonl"), "w") as f:
        for i, (F, M) in enumerate(RANK_SHAPES):
            us = sorted((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows[i * (1 + RANK_REPS) + 1:(i + 1) * (1 + RANK_REPS)])
            rec = {"kernel": "rank_quality_kernel", "F": F, "M": M, "launches": len(us), "us_median": round(us[len(us) // 2], 2), "us_min": round(us[0], 2),
                   "us_max": round(us[-1], 2)}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
    shutil.rmtree(tmp, ignore_errors=True)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="F <= 256 only")
    ap.add_argument("--parent-module", default=None, help="cvxpnpl_amd/ransac.py of another checkout: the unguided baseline")
    ap.add_argument("--rank-trace", default=None, metavar="DIR", help="kernel trace of the ranking alone, in a child process")
    ap.add_argument("--rank-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.rank_child:
        return rank_child()
    if a.rank_trace:  # this process never opens the GPU: the profiled program is a child of its own
        return rank_trace(a.rank_trace)
    import torch

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    parent_fn = None
    if a.parent_module:  # the baseline's package under another name, beside this one
        pkg = os.path.dirname(os.path.abspath(a.parent_module))
        spec = importlib.util.spec_from_file_location("cvxpnpl_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["cvxpnpl_amd_parent"] = mod
        spec.loader.exec_module(mod)
        parent_fn = mod.ransac.ransac_pnp_batch
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    recs = []
    for clutter in (0.5, 0.7):
        for F in (16, 256) if a.quick else (16, 256, 1024):
            recs.append(one_shape(F, clutter, reps=9 if F <= 16 else (5 if F <= 256 else 3), parent_fn=parent_fn))
            if a.out:
                with open(os.path.join(a.out, "rate.jsonl"), "w") as f:
                    for r in recs:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
