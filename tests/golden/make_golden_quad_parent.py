#!/usr/bin/env python3
"""Records tests/golden/quad_parent_outputs.npz: what the quad-schedule kernels (cvxq::solve_quad_kernel, csrc/quad_kernel.h) return, bit for
bit, for a handful of small seeded batches.

The fixture was recorded ON AN MI355X FROM A BUILD OF THE PARENT COMMIT'S SOURCES of the change that re-ordered the LDS reads of the
iteration's short phases (G build, W+, projection; profiles/r08/quad_lds_phases_ab.txt) -- before any edit to the kernel.  That change, and
any later one that only moves loads or interleaves independent chains, must reproduce it exactly (tests/test_quad_bitwise_gpu.py).  A change
that alters the arithmetic ON PURPOSE regenerates the fixture from ITS parent first, with this script, and says so:

    python tests/golden/make_golden_quad_parent.py [out.npz]        (GPU; the library under cvxpnpl_amd/, or CVXPNPL_AMD_LIB)

The problems come from cvxpnpl_amd.synth with fixed seeds.  Per case: status, iters, work in full; R, t, cost in full, or their SHA-256 for
the large batch (HASHED) to keep the file small.  This module is also the test's list of cases (CASES, run_case).
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "quad_parent_outputs.npz")

QUAD, PENTA = 3, 4  # CVXPNPL_LAYOUT_*
F64 = {"f32_sweeps_until": 0}  # every sweep in float64: the instantiations with F64SW = true
INTS, FLOATS = ("status", "iters", "work"), ("R", "t", "cost")

# name -> (kind, generator arguments, batch, solver options, floats hashed)
CASES = {}
for _b in (257, 259):  # a partial last wavefront: 1 and 3 of 4 rows real, the others redo the last problem
    CASES[f"n10_f64_b{_b}"] = ("pnp", dict(n=10, sigma=2.0, seed=42), _b, dict(layout=QUAD, **F64), False)      # <0,2,16,true,0>, bench.py's kernel
    CASES[f"n10_mixed_b{_b}"] = ("pnp", dict(n=10, sigma=2.0, seed=42), _b, dict(layout=QUAD), False)           # <0,2,16,false,0>
CASES["pnpl55_f64"] = ("pnpl", dict(n_p=5, n_l=5, sigma=1.0, seed=43), 131, dict(layout=QUAD, **F64), False)    # lines in the quad schedule
CASES["pnpl55_mixed"] = ("pnpl", dict(n_p=5, n_l=5, sigma=1.0, seed=43), 131, dict(layout=QUAD), False)
CASES["n6_s5_f64"] = ("pnp", dict(n=6, sigma=5.0, seed=44), 131, dict(layout=QUAD, **F64), False)               # survivors through finish_own
CASES["rc_f64"] = ("pnp", dict(n=10, sigma=2.0, seed=45), 131, dict(layout=QUAD, variant=1, **F64), False)      # quad_proj<VAR_RC>
CASES["rc_mixed"] = ("pnp", dict(n=10, sigma=2.0, seed=45), 131, dict(layout=QUAD, variant=1), False)
CASES["n4_auto_f64"] = ("pnp", dict(n=4, sigma=1.0, seed=46), 2560, dict(**F64), True)                          # the two MODE 2 kernels (AUTO: minimal problems)
CASES["n4_auto_mixed"] = ("pnp", dict(n=4, sigma=1.0, seed=46), 2560, dict(), True)
CASES["penta_mixed"] = ("pnp", dict(n=10, sigma=2.0, seed=47), 61, dict(layout=PENTA), False)                   # LPP = 12, EPL = 5
CASES["cost_seam_f64"] = ("cost", dict(n=10, sigma=2.0, seed=42), 67, dict(layout=QUAD, **F64), False)          # the Q45 entry; problems of case 1


def run_case(name, device):
    """{array name: numpy array} of one case from the library that is loaded"""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import synth

    kind, gen, batch, opts, _ = CASES[name]
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x[:batch]), device=device)  # noqa: E731
    if kind == "pnpl":
        d = synth.make_pnpl(batch, gen["n_p"], gen["n_l"], gen["sigma"], seed=gen["seed"])
        res = ca.pnpl_batch(dev(d["pts_2d"]), dev(d["line_2d"]), dev(d["pts_3d"]), dev(d["line_3d"]), torch.as_tensor(d["K"], device=device), **opts)
    else:
        # (case "cost": the first 67 problems of the 257 of case 1 -- the generator draws batch-major, so the batch it is asked for matters)
        d = synth.make_pnp(257 if kind == "cost" else batch, gen["n"], gen["sigma"], seed=gen["seed"])
        K = torch.as_tensor(d["K"], device=device)
        if kind == "cost":
            Bt, Qt = ca.assemble_batch(dev(d["pts_2d"]), None, dev(d["pts_3d"]), None, K, device=device)
            res = ca.solve_cost_batch(Qt, Bt, device=device, **opts)
        else:
            res = ca.pnp_batch(dev(d["pts_2d"]), dev(d["pts_3d"]), K, **opts)
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(res[k].cpu().numpy()) for k in INTS + FLOATS}


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def stored(name, out):
    """what the fixture keeps of a case's outputs: {"<case>__<array>": array} (floats of a HASHED case as "<case>__<array>.sha256")"""
    keep = {}
    for k in INTS:
        keep[f"{name}__{k}"] = out[k]
    for k in FLOATS:
        if CASES[name][4]:
            keep[f"{name}__{k}.sha256"] = digest(out[k])
        else:
            keep[f"{name}__{k}"] = out[k]
    return keep


def main():
    import torch

    sys.path.insert(0, ROOT)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    device = torch.device("cuda:0")
    keep = {}
    for name in CASES:
        a, b = run_case(name, device), run_case(name, device)
        for k in a:  # the record must be a function of the inputs alone
            assert a[k].tobytes() == b[k].tobytes(), f"{name}__{k}: two runs of the same library differ"
        keep.update(stored(name, a))
        print(name, "status", np.bincount(a["status"], minlength=5).tolist(), "iters", np.bincount(a["iters"]).nonzero()[0].tolist(), flush=True)
    np.savez_compressed(path, **keep)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
