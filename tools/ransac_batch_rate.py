"""Frames per second of ransac_pnp_batch against a Python loop of ransac_pnp over the same scenes, in one process.

    python tools/ransac_batch_rate.py [--out DIR] [--quick] [--profile]

Grid: F in {1, 16, 256, 1024} scenes of M = 100 correspondences, H in {256, 1024, 4096} hypotheses per scene, and one ragged set
(F = 256, M_f from 50 to 2000, H = 1024).  Scenes are on the device before the clock starts for both.  Every timed call ends in its
read-back, so device events and the wall clock bracket the same work; each shape is warmed up once, then the two are timed in alternation
and the medians are reported with the spread (min .. max) of the repeats.  One JSON line per shape; with --out also DIR/rate.jsonl.
--profile first runs, in a child process of its own, one batched call (F = 256, H = 1024, M = 100) under `rocprofv3 --kernel-trace --stats`
and keeps the kernel statistics as DIR/kernel_stats.csv.  --one F H: that child (two calls, no timing).
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scenes(F, M, seed0=0, ragged=False):
    import numpy as np

    from cvxpnpl_amd import synth

    sizes = [int(v) for v in np.round(np.geomspace(50, 2000, F))] if ragged else [M] * F
    xs, Xs = [], []
    for f, m in enumerate(sizes):
        d = synth.make_ransac(1, n_corr=m, outlier_frac=0.3, sigma=0.5, seed=seed0 + f)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"])
    return xs, Xs, synth.K_KINECT


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, time.perf_counter() - w


def one_shape(F, H, M, reps, ragged=False):
    import torch

    from cvxpnpl_amd import ransac

    dev = torch.device("cuda:0")
    xs, Xs, K = scenes(F, M, ragged=ragged)
    x = [torch.as_tensor(a, device=dev) for a in xs]
    X = [torch.as_tensor(a, device=dev) for a in Xs]
    Kd = torch.as_tensor(K, device=dev)
    xp, Xp, sizes = torch.cat(x), torch.cat(X), [a.shape[0] for a in x]

    def batched():
        return ransac.ransac_pnp_batch(xp, Xp, Kd, n_hyp=H, seed=0, sizes=sizes, device=dev)

    def loop():
        return [ransac.ransac_pnp(x[f], X[f], Kd, n_hyp=H, seed=f, device=dev) for f in range(F)]

    out, ref = batched(), loop()  # warm-up of both at this shape, and the result check: the same consensus up to borderline pixels
    agree = sum(abs(int(out["n_inliers"][f]) - ref[f]["n_inliers"]) <= 1 for f in range(F))
    tb, tl = [], []
    for _ in range(reps):  # alternating
        tb.append(timed(batched))
        tl.append(timed(loop))
    med = lambda v, k: sorted(t[k] for t in v)[len(v) // 2]  # noqa: E731
    rec = {"F": F, "H": H, "M": "50..2000" if ragged else M, "reps": reps,
           "batch_fps_events": round(F / med(tb, 0), 1), "loop_fps_events": round(F / med(tl, 0), 1),
           "batch_fps_wall": round(F / med(tb, 1), 1), "loop_fps_wall": round(F / med(tl, 1), 1),
           "ratio_wall": round(med(tl, 1) / med(tb, 1), 2),
           "batch_ms_min_max": [round(min(t[1] for t in tb) * 1e3, 3), round(max(t[1] for t in tb) * 1e3, 3)],
           "loop_ms_min_max": [round(min(t[1] for t in tl) * 1e3, 3), round(max(t[1] for t in tl) * 1e3, 3)],
           "scenes_with_same_consensus": agree}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="F <= 256 only")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--one", nargs=2, type=int, default=None, metavar=("F", "H"))
    a = ap.parse_args(argv)
    if a.one:
        import torch

        from cvxpnpl_amd import ransac

        xs, Xs, K = scenes(a.one[0], 100)
        for _ in range(2):
            ransac.ransac_pnp_batch(xs, Xs, K, n_hyp=a.one[1], seed=0, device=torch.device("cuda:0"))
        return
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.profile:  # before this process opens the GPU: the profiled program is a child of its own
        tmp = os.path.join(a.out or ".", "_rocprof")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "ransac_batch", "--", sys.executable, os.path.abspath(__file__),
                            "--one", "256", "1024"], timeout=600)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            raise SystemExit(f"rocprofv3 run failed ({r.returncode})")
        if a.out:
            shutil.copy(stats[0], os.path.join(a.out, "kernel_stats.csv"))
            shutil.rmtree(tmp, ignore_errors=True)
    import torch

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    recs = []
    for F in (1, 16, 256) if a.quick else (1, 16, 256, 1024):
        for H in (256, 1024, 4096):
            recs.append(one_shape(F, H, 100, reps=11 if F <= 16 else (5 if F <= 256 else 3)))
    recs.append(one_shape(256, 1024, 0, reps=5, ragged=True))
    if a.out:
        with open(os.path.join(a.out, "rate.jsonl"), "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
