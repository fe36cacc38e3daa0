#!/usr/bin/env python3
"""Generate tests/golden/recover_planted.npz: planted multi-pose solutions and what the REFERENCE makes of them.

Run in the build container only (the GPU box has no /root/reference):

    python -B tests/golden/make_golden_recover.py [--check]

The problems come from tests/recover_reference.py (numpy only, from the seeds below).  The reference module is imported
with a stub `scs` the way tests/golden/make_golden.py does: the stub's solve() hands the planted Z back as the solver's
answer and the reference's own _solve_relaxation does the rest.  Of the reference only outputs are stored: the rotations it
returns (its _constraint_ortho_det rows projected by SVD), per problem.  What follows from the stored arrays is not stored
again: Z of the exact classes is plant_Z(R, w), the reference's error is rot_err of its rotations against the planted ones
(recover_reference.load_fixture rebuilds both).  No reference source text is copied.  Always run with -B.

The archive is written with fixed member timestamps, so the same seeds give the same file bit for bit; --check compares
with the committed file instead of writing.
"""
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recover_reference as rr  # noqa: E402

stub = types.ModuleType("scs")
stub.__version__ = "3.2.4"
sys.modules["scs"] = stub
sys.path.insert(0, "/root/reference")
_HAD_CACHE = os.path.exists("/root/reference/__pycache__")
import cvxpnpl as ref  # noqa: E402

SEED = 20261018


def _solve(data, cones, **kw):
    return {"x": np.array(_inject["x"], dtype=np.float64), "info": {"dobj": 0.0}}


_inject = {"x": None}
stub.solve = _solve


def reference_poses(Z55):
    """The rotations the reference's own _solve_relaxation returns when its solver hands back x = Z55 (the cost plays no part in
    what follows the solve; a zero one is passed).  One NaN pose where the reference produces NaN."""
    _inject["x"] = Z55
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            poses = ref._solve_relaxation(np.zeros((1, 9)), np.zeros((3, 9)))
        except np.linalg.LinAlgError:
            return np.full((1, 3, 3), np.nan)
    return np.stack([p[0] for p in poses])


def draw(name, rs):
    """One candidate problem of a class: (Rs, w, Z (10x10))."""
    k = rr.CLASSES[name][0]
    if name.startswith("k2_rand") or name.startswith("k4_rand"):
        Rs = rr.rotations_random(rs, k)
        w = rr.weights(rs, k, 0.25 if name.endswith("w25") else 0.02)
    elif name.startswith("k2_twin"):
        Rs = rr.rotations_twins(rs, {"05": 0.5, "02": 0.2, "01": 0.1}[name[-2:]])
        w = rr.weights(rs, 2, 0.25)
    elif name.startswith("planar"):
        Rs = rr.rotations_planar(rs)
        w = np.array([0.5, 0.5]) if name == "planar_eq" else np.array([0.7, 0.3])
    elif name == "k4_near":
        Rs = rr.rotations_near(rs, 4, 0.5)
        w = rr.weights(rs, 4, 0.25)
    elif name in rr.POLISHED or name in rr.RANK1 or name in rr.ODD:
        Rs = rr.rotations_random(rs, k)
        w = rr.weights(rs, k, 0.25)
    elif name in rr.THRESHOLD:
        Rs = rr.rotations_random(rs, 2)
        w = rr.second_weight_for(Rs, 2e-3 if name == "thr_hi" else 5e-4)
    else:
        raise KeyError(name)
    Z = rr.plant_Z(Rs, w)
    if name.endswith("_noise"):
        Z = Z + rr.sym_noise(rs, 1e-8)
    if name == "r1_pert":
        Z = Z + rr.sym_noise(rs, 1e-5)
    return Rs, w, Z


def make_class(name, seed):
    k, n = rr.CLASSES[name]
    rs = np.random.RandomState(seed)
    want_rank = {"thr_lo": 1}.get(name, k)
    out = {key: [] for key in ("Z55", "R", "w", "B27", "ref_R", "ref_n", "ref_err")}
    if name in rr.POLISHED:
        out["Q45"] = []
    redraws = 0
    while len(out["Z55"]) < n:
        Rs, w, Z = draw(name, rs)
        Z55 = ref._vech10(Z)
        assert np.array_equal(Z55, rr.vech10(Z))  # the helper packs in the reference's order
        # from numpy alone: no eigenvalue near the rank threshold, and the rank that the class is meant to have
        if rr.rank_margin(Z55) < rr.RANK_MARGIN or rr.np_rank(Z55) != want_rank:
            redraws += 1
            assert redraws < 50 * n, name
            continue
        B27 = rr.rand_B27(rs)
        if name in rr.POLISHED:
            for _ in range(100):
                Q = rr.polish_Q(Rs, rs)
                if rr.hessian_cond(Q, Rs) <= rr.KAPPA_MAX:
                    break
            else:
                raise AssertionError(f"{name}: no polish cost with Hessian condition <= {rr.KAPPA_MAX}")
            out["Q45"].append(rr.pack_q45(Q))
        Rr = reference_poses(Z55)
        err = rr.rot_err(Rr, Rs)[0] if np.isfinite(Rr).all() else np.nan
        pad = np.full((4, 3, 3), np.nan)
        pad[:len(Rr)] = Rr
        for key, val in (("Z55", Z55), ("R", Rs), ("w", w), ("B27", B27), ("ref_R", pad), ("ref_n", len(Rr)), ("ref_err", err)):
            out[key].append(val)
    out = {key: np.asarray(val) for key, val in out.items()}
    out["ref_n"] = out["ref_n"].astype(np.int32)
    stored = {key: val for key, val in out.items() if key != "ref_err" and (key != "Z55" or name in rr.STORED_Z)}
    back = rr.complete_class(name, dict(stored))  # what load_fixture will hand to the tests
    assert all(np.array_equal(back[key], out[key], equal_nan=True) for key in out), name
    if name in rr.UNPOLISHED_K4:  # a condition on the fixture: the problems held to DESIGN_BOUND instead of the reference
        share = float((out["ref_err"] > rr.DESIGN_BOUND).mean())
        assert share <= 0.10, (name, share)
    return out, stored, redraws


def archive(arrays):
    """An .npz (deflated) with fixed member timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, member.getvalue())
    return buf.getvalue()


def main():
    G = {}
    seeds = {name: SEED + i for i, name in enumerate(rr.CLASSES)}
    seeds["thr_lo"] = seeds["thr_hi"]  # pairs: the same two rotations and B, another second weight
    for name in rr.CLASSES:
        cls, stored, redraws = make_class(name, seeds[name])
        e = cls["ref_err"]
        print(f"{name:16s} n={len(e):3d} redraws={redraws:3d} reference: NaN on {int(np.isnan(e).sum()):2d}, "
              f"max {np.nanmax(e):.2e} median {np.nanmedian(e):.2e}, above 1e-6: {int((e > 1e-6).sum())}")
        for key, val in stored.items():
            G[f"{name}__{key}"] = val
    assert np.array_equal(G["thr_hi__R"], G["thr_lo__R"]) and np.array_equal(G["thr_hi__B27"], G["thr_lo__B27"])
    blob = archive(G)
    if "--check" in sys.argv:
        assert open(rr.FIXTURE, "rb").read() == blob, "the committed fixture differs from what the seeds give"
        print("fixture reproduced bit for bit:", len(blob), "bytes")
    else:
        with open(rr.FIXTURE, "wb") as f:
            f.write(blob)
        print("wrote", rr.FIXTURE, "with", len(G), "arrays,", len(blob), "bytes")
    assert _HAD_CACHE or not os.path.exists("/root/reference/__pycache__"), "bytecode leaked into the reference tree"


if __name__ == "__main__":
    main()
