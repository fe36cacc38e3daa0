"""Frames per second of ransac_pnpl_batch(confidence=0.99) and of its guided draws against the fixed budget n_hyp = cap, in one process.

    python tools/ransac_pnpl_adaptive_rate.py [--out DIR] [--quick] [--fixed-module PATH]
    python tools/ransac_pnpl_adaptive_rate.py --kernel-share DIR

Grid: F in {1, 16, 256, 1024} scenes of 100 points + 50 lines, cap in {256, 1024}, round_hyp in {32, 64, 256}, on two scene sets: "0.3"
(every scene 30 % clutter) and "mixed" (clutter shares spread over 0 .. 0.6).  Then a guided leg at 50 % and 70 % clutter, F in {16, 256},
cap 1024, rounds of 64: the adaptive call unguided, guided by an informative quality (U(0.2, 1) on the inliers, U(0, 0.8) on the clutter,
points and lines on that one scale) and guided by the same quality reversed.  The method is that of tools/ransac_adaptive_rate.py: scenes
are on the device before the clock starts, every timed call ends in its read-back, each shape is warmed up once, the calls are timed in
alternation, and medians are reported with the spread (min .. max) of the repeats.  The fixed call is the same function without the
keywords; --fixed-module PATH loads cvxpnpl_amd/ransac.py of another checkout for it instead (its libraries must be built), to time the
parent commit itself.  Also reported per shape: hypotheses solved in all, rounds, ms per round, and the quality against the fixed call
at the cap.  One JSON line per shape; with --out also DIR/rate.jsonl.

--kernel-share DIR: the share of every kernel in one adaptive call (mixed set, F = 256, cap 1024, rounds of 64).  The call runs in a child
process of its own under `rocprofv3 --kernel-trace`, after one warm-up; the kernels of the second call are read from the trace, summed
by name and written to DIR/kernel_share.jsonl.
"""
import argparse
import glob
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUND_HYP = (32, 64, 256)
P, L = 100, 50


def scenes(F, kind, seed0=0):
    """packed device arrays (p2, l2, p3, l3), K and the ground-truth inlier flags (points, lines), packed"""
    import numpy as np
    import torch

    from cvxpnpl_amd import synth

    if isinstance(kind, float):
        shares = [kind] * F
    else:
        shares = [0.3] * F if kind == "0.3" else ([0.3] if F == 1 else list(np.linspace(0.0, 0.6, F)))
    ds = [synth.make_ransac_pnpl(P, L, outlier_frac=float(shares[f]), sigma=0.5, seed=seed0 + f) for f in range(F)]
    dev = torch.device("cuda:0")
    packed = [torch.as_tensor(np.concatenate([d[k] for d in ds]), device=dev) for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")]
    return packed, torch.as_tensor(synth.K_KINECT, device=dev), np.concatenate([d["inlier_pts"] for d in ds]), np.concatenate([d["inlier_lines"] for d in ds])


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


def _ms(v):
    return [round(min(t[1] for t in v) * 1e3, 3), round(max(t[1] for t in v) * 1e3, 3)]


def _quality(out, ref):
    """share of the scenes where the fixed call at the cap reaches a consensus: pose within 1e-3 rad of it, inliers >= 0.95 of its"""
    from cvxpnpl_amd import synth

    nf = ref["n_inliers"].numpy()
    ok = nf >= 4
    if not ok.any():
        return {}
    geo = synth.geodesic(out["R"].cpu().numpy()[ok], ref["R"].cpu().numpy()[ok])
    return {"pose_within_1e-3_rad": round(float((geo < 1e-3).mean()), 4),
            "inliers_at_least_0.95": round(float((out["n_inliers"].numpy()[ok] >= 0.95 * nf[ok]).mean()), 4)}


def _row(F, times, t_fixed, out, ref):
    ms = _med(times, 1) * 1e3
    r = {"fps_wall": round(F / _med(times, 1), 1), "fps_events": round(F / _med(times, 0), 1), "ms_min_max": _ms(times),
         "hyp": int(out["hyp_used"].sum()), "rounds": out["rounds"], "ms_per_round": round(ms / out["rounds"], 3),
         "speedup_wall": round(_med(t_fixed, 1) / _med(times, 1), 2)}
    r.update(_quality(out, ref))
    return r


def one_shape(F, cap, kind, reps, fixed_fn):
    from cvxpnpl_amd import ransac

    (p2, l2, p3, l3), K, _, _ = scenes(F, kind)
    kw = dict(n_hyp=cap, seed=0, sizes=[P] * F, line_sizes=[L] * F, device=K.device)

    def fixed():
        return fixed_fn(p2, l2, p3, l3, K, **kw)

    def none():
        return ransac.ransac_pnpl_batch(p2, l2, p3, l3, K, confidence=None, quality=None, line_quality=None, **kw)

    def adaptive(rh):
        return lambda: ransac.ransac_pnpl_batch(p2, l2, p3, l3, K, confidence=0.99, round_hyp=rh, **kw)

    rhs = [rh for rh in ROUND_HYP if rh <= cap]
    ref = fixed()  # warm-up of everything at this shape
    none()
    for rh in rhs:
        adaptive(rh)()
    tf, tn, ta = [], [], {rh: [] for rh in rhs}
    for _ in range(reps):  # alternating
        tf.append(timed(fixed))
        for rh in rhs:
            ta[rh].append(timed(adaptive(rh)))
        tn.append(timed(none))
    rec = {"leg": "adaptive", "F": F, "cap": cap, "P": P, "L": L, "set": kind, "reps": reps, "fixed_hyp": F * cap,
           "fixed_fps_wall": round(F / _med(tf, 1), 1), "fixed_fps_events": round(F / _med(tf, 0), 1), "fixed_ms_min_max": _ms(tf),
           "none_fps_wall": round(F / _med(tn, 1), 1), "none_ms_min_max": _ms(tn),
           "adaptive": {str(rh): _row(F, ta[rh], tf, ta[rh][-1][2], ref) for rh in rhs}}
    print(json.dumps(rec), flush=True)
    return rec


def guided_shape(F, cap, clutter, reps, fixed_fn, rh=64):
    import numpy as np
    import torch

    from cvxpnpl_amd import ransac

    (p2, l2, p3, l3), K, ip, il = scenes(F, float(clutter), seed0=5000)
    rs = np.random.RandomState(11)
    qp = np.where(ip, rs.uniform(0.2, 1.0, len(ip)), rs.uniform(0.0, 0.8, len(ip)))
    ql = np.where(il, rs.uniform(0.2, 1.0, len(il)), rs.uniform(0.0, 0.8, len(il)))
    dev = K.device
    priors = {"informative": (torch.as_tensor(qp, device=dev), torch.as_tensor(ql, device=dev)),
              "reversed": (torch.as_tensor(-qp, device=dev), torch.as_tensor(-ql, device=dev))}
    kw = dict(n_hyp=cap, seed=0, sizes=[P] * F, line_sizes=[L] * F, device=dev)

    def fixed():
        return fixed_fn(p2, l2, p3, l3, K, **kw)

    def call(prior):
        q = {} if prior is None else dict(quality=priors[prior][0], line_quality=priors[prior][1])
        return lambda: ransac.ransac_pnpl_batch(p2, l2, p3, l3, K, confidence=0.99, round_hyp=rh, **q, **kw)

    legs = {"unguided": call(None), "informative": call("informative"), "reversed": call("reversed")}
    ref = fixed()
    for fn in legs.values():
        fn()
    tf, tl = [], {k: [] for k in legs}
    for _ in range(reps):
        tf.append(timed(fixed))
        for k, fn in legs.items():
            tl[k].append(timed(fn))
    rec = {"leg": "guided", "F": F, "cap": cap, "P": P, "L": L, "clutter": clutter, "round_hyp": rh, "reps": reps, "fixed_hyp": F * cap,
           "fixed_fps_wall": round(F / _med(tf, 1), 1), "fixed_ms_min_max": _ms(tf),
           "calls": {k: _row(F, tl[k], tf, tl[k][-1][2], ref) for k in legs}}
    print(json.dumps(rec), flush=True)
    return rec


SHARE_SHAPE = (256, 1024, 64)  # F, cap, round_hyp of --kernel-share


def share_child():
    """The launches of --kernel-share: one warm-up call and one call, told apart in the trace by a marker kernel (a fill of 12345 bytes)."""
    import torch

    from cvxpnpl_amd import ransac

    F, cap, rh = SHARE_SHAPE
    (p2, l2, p3, l3), K, _, _ = scenes(F, "mixed")
    kw = dict(n_hyp=cap, seed=0, sizes=[P] * F, line_sizes=[L] * F, device=K.device, confidence=0.99, round_hyp=rh)
    ransac.ransac_pnpl_batch(p2, l2, p3, l3, K, **kw)
    torch.cuda.synchronize()
    torch.empty(12345, dtype=torch.uint8, device=K.device).fill_(1)
    torch.cuda.synchronize()
    out = ransac.ransac_pnpl_batch(p2, l2, p3, l3, K, **kw)
    torch.cuda.synchronize()
    print(json.dumps({"hyp": int(out["hyp_used"].sum()), "rounds": out["rounds"]}), flush=True)


def kernel_share(out):
    import csv

    os.makedirs(out, exist_ok=True)
    tmp = os.path.join(out, "_rocprof_share")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "share", "--", sys.executable,
                        os.path.abspath(__file__), "--share-child"], timeout=600)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not found:
        raise SystemExit(f"rocprofv3 run failed ({r.returncode})")
    rows = [row for f in found for row in csv.DictReader(open(f))]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    fills = [i for i, row in enumerate(rows) if "fill" in row["Kernel_Name"].lower() or "Fill" in row["Kernel_Name"]]
    assert fills, "the marker kernel is not in the trace"
    mark = min(fills, key=lambda i: abs(i - len(rows) // 2))  # the two calls launch the same kernels: the marker sits in the middle
    rows = rows[mark + 1:]  # the second call
    tot, by = 0, {}
    for row in rows:
        dt = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        name = row["Kernel_Name"].split("(")[0].replace("void ", "")
        n, t = by.get(name, (0, 0))
        by[name] = (n + 1, t + dt)
        tot += dt
    span = int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])
    F, cap, rh = SHARE_SHAPE
    with open(os.path.join(out, "kernel_share.jsonl"), "w") as f:
        head = {"F": F, "cap": cap, "round_hyp": rh, "set": "mixed", "kernel_us": round(tot * 1e-3, 1), "first_to_last_us": round(span * 1e-3, 1)}
        f.write(json.dumps(head) + "\n")
        print(json.dumps(head))
        for name, (n, t) in sorted(by.items(), key=lambda kv: -kv[1][1]):
            rec = {"kernel": name, "launches": n, "us": round(t * 1e-3, 1), "share": round(t / tot, 4)}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="F <= 256 only")
    ap.add_argument("--fixed-module", default=None, help="cvxpnpl_amd/ransac.py of another checkout: the fixed-budget baseline")
    ap.add_argument("--kernel-share", default=None, metavar="DIR", help="kernel trace of one adaptive call, in a child process")
    ap.add_argument("--share-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.share_child:
        return share_child()
    if a.kernel_share:  # this process never opens the GPU: the profiled program is a child of its own
        return kernel_share(a.kernel_share)
    import torch

    from cvxpnpl_amd import ransac

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    fixed_fn = ransac.ransac_pnpl_batch
    if a.fixed_module:  # the baseline's package under another name, beside this one
        pkg = os.path.dirname(os.path.abspath(a.fixed_module))
        spec = importlib.util.spec_from_file_location("cvxpnpl_amd_fixed", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["cvxpnpl_amd_fixed"] = mod
        spec.loader.exec_module(mod)
        fixed_fn = mod.ransac.ransac_pnpl_batch
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    recs = []

    def keep(rec):
        recs.append(rec)
        if a.out:
            with open(os.path.join(a.out, "rate.jsonl"), "w") as f:
                for r in recs:
                    f.write(json.dumps(r) + "\n")

    for kind in ("0.3", "mixed"):
        for F in (1, 16, 256) if a.quick else (1, 16, 256, 1024):
            for cap in (256, 1024):
                keep(one_shape(F, cap, kind, reps=9 if F <= 16 else (5 if F <= 256 else 3), fixed_fn=fixed_fn))
    for clutter in (0.5, 0.7):
        for F in (16, 256):
            keep(guided_shape(F, 1024, clutter, reps=5, fixed_fn=fixed_fn))


if __name__ == "__main__":
    main(sys.argv[1:])
