"""Frames per second of ransac_pnpl_batch against a Python loop of ransac_pnpl over the same scenes, and -- on point-only scenes -- against
ransac_pnp_batch of the same checkout, in one process.

    python tools/ransac_pnpl_rate.py [--out DIR] [--profile]

Grid: F in {1, 16, 256} scenes of 100 points + 50 lines, H in {256, 1024} hypotheses per scene; the same grid with 100 points and no
lines for the comparison with ransac_pnp_batch (what routing the minimal solves through the cost seam costs or saves).  Scenes are on
the device before the clock starts.  Every timed call ends in its read-back; each shape is warmed up once, then the contenders are timed
in alternation and the median is reported with the spread (min .. max) of the repeats.  One JSON line per shape; with --out also
DIR/rate.jsonl.  --profile first runs, in a child process of its own, one batched call (F = 256, H = 1024) under
`rocprofv3 --kernel-trace --stats` and keeps the kernel statistics as DIR/kernel_stats.csv.  --one F H: that child (two calls).
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


def scenes(F, P, L, dev, seed0=0):
    import torch

    from cvxpnpl_amd import synth

    fr = [synth.make_ransac_pnpl(P, L, outlier_frac=0.3, sigma=0.5, seed=seed0 + f) for f in range(F)]
    t = lambda k: [torch.as_tensor(d[k], device=dev) for d in fr]  # noqa: E731
    return t("pts_2d"), t("line_2d"), t("pts_3d"), t("line_3d"), torch.as_tensor(synth.K_KINECT, device=dev)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    w = time.perf_counter()
    fn()   # (ends in its read-back)
    return time.perf_counter() - w


def stats(v, F):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2] * 1e3, 3), "ms_min": round(v[0] * 1e3, 3), "ms_max": round(v[-1] * 1e3, 3), "fps_median": round(F / v[len(v) // 2], 1)}


def one_shape(F, H, P, L, reps):
    import torch

    from cvxpnpl_amd import ransac

    dev = torch.device("cuda:0")
    x, l2, X, l3, K = scenes(F, P, L, dev)
    xp, Xp = torch.cat(x), torch.cat(X)
    l2p, l3p = (torch.cat(l2), torch.cat(l3)) if L else (None, None)
    contenders = {"pnpl_batch": lambda: ransac.ransac_pnpl_batch(xp, l2p, Xp, l3p, K, n_hyp=H, seed=0, sizes=[P] * F, line_sizes=[L] * F if L else None, device=dev)}
    if L:
        contenders["pnpl_loop"] = lambda: [ransac.ransac_pnpl(x[f], l2[f], X[f], l3[f], K, n_hyp=H, seed=f, device=dev) for f in range(F)]
    else:
        contenders["pnp_batch"] = lambda: ransac.ransac_pnp_batch(xp, Xp, K, n_hyp=H, seed=0, sizes=[P] * F, device=dev)
    first = {k: fn() for k, fn in contenders.items()}   # warm-up of every contender at this shape, and the result check
    rec = {"F": F, "H": H, "P": P, "L": L, "reps": reps}
    if L:
        rec["scenes_with_same_consensus"] = sum(abs(int(first["pnpl_batch"]["n_inliers"][f]) - first["pnpl_loop"][f]["n_inliers"]) <= 1 for f in range(F))
    else:
        rec["scenes_with_same_consensus"] = int((first["pnpl_batch"]["n_inliers"] == first["pnp_batch"]["n_inliers"]).sum())
    times = {k: [] for k in contenders}
    for _ in range(reps):  # alternating
        for k, fn in contenders.items():
            times[k].append(timed(fn))
    for k in contenders:
        rec[k] = stats(times[k], F)
    other = "pnpl_loop" if L else "pnp_batch"
    rec[f"{other}_over_pnpl_batch"] = round(rec[other]["ms_median"] / rec["pnpl_batch"]["ms_median"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--one", nargs=2, type=int, default=None, metavar=("F", "H"))
    a = ap.parse_args(argv)
    if a.one:
        import torch

        from cvxpnpl_amd import ransac

        dev = torch.device("cuda:0")
        x, l2, X, l3, K = scenes(a.one[0], 100, 50, dev)
        for _ in range(2):
            ransac.ransac_pnpl_batch(x, l2, X, l3, K, n_hyp=a.one[1], seed=0, device=dev)
        return
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.profile:  # before this process opens the GPU: the profiled program is a child of its own
        tmp = os.path.join(a.out or ".", "_rocprof_pnpl")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "ransac_pnpl", "--", sys.executable,
                            os.path.abspath(__file__), "--one", "256", "1024"], timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            raise SystemExit(f"rocprofv3 run failed ({r.returncode})")
        if a.out:
            shutil.copy(found[0], os.path.join(a.out, "kernel_stats.csv"))
            shutil.rmtree(tmp, ignore_errors=True)
    import torch

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    recs = []
    for L in (50, 0):
        for F in (1, 16, 256):
            for H in (256, 1024):
                recs.append(one_shape(F, H, 100, L, reps=11 if F <= 16 else 5))
    if a.out:
        with open(os.path.join(a.out, "rate.jsonl"), "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
