"""Frames per second of ransac_pnp_batch(confidence=0.99), the budget per scene, against the fixed budget n_hyp = cap, in one process.

    python tools/ransac_adaptive_rate.py [--out DIR] [--quick] [--fixed-module PATH]

Grid: F in {1, 16, 256, 1024} scenes of M = 100 correspondences, cap in {256, 1024, 4096}, round_hyp in {32, 64, 256}, on two scene
sets: "0.3" (every scene 30 % clutter, the README's scene) and "mixed" (clutter shares spread over 0 .. 0.6).  The method is that of
tools/ransac_batch_rate.py: scenes are on the device before the clock starts, every timed call ends in its read-back, each shape is
warmed up once, the adaptive calls and the fixed call are timed in alternation, and medians are reported with the spread (min .. max) of
the repeats.  The fixed call is the same function without `confidence` -- the code path of the parent commit; --fixed-module PATH loads
cvxpnpl_amd/ransac.py of another checkout for it instead (its libraries must be built), to time the parent commit itself.  Also
reported per shape: hypotheses solved in all, rounds, ms per round, and on the mixed set the quality against the fixed call at the cap.
One JSON line per shape; with --out also DIR/rate.jsonl.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUND_HYP = (32, 64, 256)


def scenes(F, kind, M=100, seed0=0):
    import numpy as np

    from cvxpnpl_amd import synth

    shares = [0.3] * F if kind == "0.3" else ([0.3] if F == 1 else list(np.linspace(0.0, 0.6, F)))
    xs, Xs = [], []
    for f in range(F):
        d = synth.make_ransac(1, n_corr=M, outlier_frac=float(shares[f]), sigma=0.5, seed=seed0 + f)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"])
    return xs, Xs, synth.K_KINECT


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


def one_shape(F, cap, kind, reps, fixed_fn):
    import numpy as np
    import torch

    from cvxpnpl_amd import ransac, synth

    dev = torch.device("cuda:0")
    xs, Xs, K = scenes(F, kind)
    xp = torch.cat([torch.as_tensor(a, device=dev) for a in xs])
    Xp = torch.cat([torch.as_tensor(a, device=dev) for a in Xs])
    Kd, sizes = torch.as_tensor(K, device=dev), [a.shape[0] for a in xs]

    def fixed():
        return fixed_fn(xp, Xp, Kd, n_hyp=cap, seed=0, sizes=sizes, device=dev)

    def none():
        return ransac.ransac_pnp_batch(xp, Xp, Kd, n_hyp=cap, seed=0, sizes=sizes, device=dev, confidence=None)

    def adaptive(rh):
        return lambda: ransac.ransac_pnp_batch(xp, Xp, Kd, n_hyp=cap, seed=0, sizes=sizes, device=dev, confidence=0.99, round_hyp=rh)

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
    rec = {"F": F, "cap": cap, "M": 100, "set": kind, "reps": reps, "fixed_hyp": F * cap,
           "fixed_fps_wall": round(F / _med(tf, 1), 1), "fixed_fps_events": round(F / _med(tf, 0), 1),
           "fixed_ms_min_max": [round(min(t[1] for t in tf) * 1e3, 3), round(max(t[1] for t in tf) * 1e3, 3)],
           "none_fps_wall": round(F / _med(tn, 1), 1),
           "none_ms_min_max": [round(min(t[1] for t in tn) * 1e3, 3), round(max(t[1] for t in tn) * 1e3, 3)], "adaptive": {}}
    Rf, nf = ref["R"].cpu().numpy(), ref["n_inliers"].numpy()
    for rh in rhs:
        out = ta[rh][-1][2]
        ms = _med(ta[rh], 1) * 1e3
        r = {"fps_wall": round(F / _med(ta[rh], 1), 1), "fps_events": round(F / _med(ta[rh], 0), 1),
             "ms_min_max": [round(min(t[1] for t in ta[rh]) * 1e3, 3), round(max(t[1] for t in ta[rh]) * 1e3, 3)],
             "hyp": int(out["hyp_used"].sum()), "rounds": out["rounds"], "ms_per_round": round(ms / out["rounds"], 3),
             "speedup_wall": round(_med(tf, 1) / _med(ta[rh], 1), 2)}
        ok = nf >= 4  # quality: over the scenes where the fixed call at the cap reaches a consensus
        if ok.any():
            geo = synth.geodesic(out["R"].cpu().numpy()[ok], Rf[ok])
            r["pose_within_1e-3_rad"] = round(float((geo < 1e-3).mean()), 4)
            r["inliers_at_least_0.95"] = round(float((out["n_inliers"].numpy()[ok] >= 0.95 * nf[ok]).mean()), 4)
        rec["adaptive"][str(rh)] = r
    print(json.dumps(rec), flush=True)
    return rec


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="F <= 256 and cap <= 1024 only")
    ap.add_argument("--fixed-module", default=None, help="cvxpnpl_amd/ransac.py of another checkout: the fixed-budget baseline")
    a = ap.parse_args(argv)
    import torch

    from cvxpnpl_amd import ransac

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    fixed_fn = ransac.ransac_pnp_batch
    if a.fixed_module:  # the baseline's package under another name, beside this one
        pkg = os.path.dirname(os.path.abspath(a.fixed_module))
        spec = importlib.util.spec_from_file_location("cvxpnpl_amd_fixed", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["cvxpnpl_amd_fixed"] = mod
        spec.loader.exec_module(mod)
        fixed_fn = mod.ransac.ransac_pnp_batch
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    recs = []
    for kind in ("0.3", "mixed"):
        for F in (1, 16, 256) if a.quick else (1, 16, 256, 1024):
            for cap in (256, 1024) if a.quick else (256, 1024, 4096):
                recs.append(one_shape(F, cap, kind, reps=9 if F <= 16 else (5 if F <= 256 else 3), fixed_fn=fixed_fn))
                if a.out:
                    with open(os.path.join(a.out, "rate.jsonl"), "w") as f:
                        for r in recs:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
