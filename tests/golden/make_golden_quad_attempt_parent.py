#!/usr/bin/env python3
"""Records tests/golden/quad_attempt_parent_outputs.npz: what the quad-schedule kernels (cvxq::solve_quad_kernel, csrc/quad_kernel.h) return,
bit for bit, for small seeded batches in which CERTIFICATE ATTEMPTS FAIL -- the cases tests/golden/make_golden_quad_parent.py does not have:
there nearly every problem is certified at its first attempt, so the LDL^T of the attempt hardly ever meets a non-positive pivot and the
polish hardly ever runs a second time.

The fixture was recorded ON AN MI355X FROM A BUILD OF THE PARENT COMMIT'S SOURCES of the change that keeps the LDS reads of the attempt in
flight (quad_ldl's pivot rows, the Newton polish; profiles/r09/quad_attempt_lds_ab.txt) -- before any edit to the kernel.  That change, and any
later one that only moves loads or replaces a branch by a select, must reproduce it exactly (tests/test_quad_attempt_bitwise_gpu.py).  A change
that alters the arithmetic ON PURPOSE regenerates the fixture from ITS parent first, with this script, and says so:

    python tests/golden/make_golden_quad_attempt_parent.py [out.npz]        (GPU; the library under cvxpnpl_amd/, or CVXPNPL_AMD_LIB)

Cases (every one with the SDP solution Z requested, every sweep in float64):
  * six points at a pixel noise at which attempts fail, batches 61 and 67 (a partial last wavefront), the full relaxation and the rc variant.
    The noise is the first of NOISE_LEVELS at which at least 10 % of the problems of the case run past the first attempt; it is found here,
    asserted here and kept in the fixture ("<case>__sigma"), which is where the test takes it from;
  * four points, 2 563 problems: the MODE 2 kernel of minimal problems (<2,2,16,true,0>), whose survivors are all queued;
  * the cost seam (cvxpnpl_solve_cost_batch) with three indefinite costs and one holding a NaN: pivots that are negative, zero or NaN, on
    which quad_ldl does not stop.  At least one status other than certified, asserted here.
Per case: status, iters, work in full; R, t, cost, Z in full, or their SHA-256 for the large batch (HASHED) to keep the file small.  This
module is also the test's list of cases (CASES, run_case).
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "quad_attempt_parent_outputs.npz")

QUAD = 3  # CVXPNPL_LAYOUT_QUAD
ST_CERTIFIED = 0
F64 = {"f32_sweeps_until": 0}  # every sweep in float64: the instantiations with F64SW = true
INTS, FLOATS = ("status", "iters", "work"), ("R", "t", "cost", "Z")
NOISE_LEVELS = (2.0, 5.0, 8.0, 12.0)  # pixels
NOISY_SHARE = 0.10

# name -> (kind, generator arguments, batch, solver options, floats hashed, iteration of the first attempt (noisy cases) or None)
CASES = {}
for _b in (61, 67):  # 1 and 3 of the 4 rows of the last wavefront real, the others redo the last problem
    CASES[f"n6_noisy_f64_b{_b}"] = ("pnp", dict(n=6, seed=50 + _b), _b, dict(layout=QUAD, **F64), False, 5)                  # <0,2,16,true,0>
    CASES[f"n6_noisy_rc_f64_b{_b}"] = ("pnp", dict(n=6, seed=60 + _b), _b, dict(layout=QUAD, variant=1, **F64), False, 19)   # <0,2,16,true,1>
CASES["n4_minimal_f64"] = ("pnp", dict(n=4, sigma=1.0, seed=48), 2563, dict(**F64), True, None)                              # <2,2,16,true,0>
CASES["cost_seam_indefinite_f64"] = ("cost", dict(n=10, sigma=2.0, seed=49), 67, dict(layout=QUAD, **F64), False, None)

INDEFINITE = {3: 0, 17: 4, 40: 8}  # cost-seam case: problem -> diagonal entry k whose Q[k][k] loses half the trace (negative afterwards, trace still > 0)
NAN_AT = (29, 7)                   # cost-seam case: (problem, packed entry) that holds a NaN


def noisy(name):
    return CASES[name][5] is not None


def run_case(name, device, sigma=None):
    """{array name: numpy array} of one case from the library that is loaded; sigma: the pixel noise of a noisy case"""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import synth

    kind, gen, batch, opts, _, _ = CASES[name]
    sig = float(sigma) if noisy(name) else gen["sigma"]
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x[:batch]), device=device)  # noqa: E731
    d = synth.make_pnp(batch, gen["n"], sig, seed=gen["seed"])
    K = torch.as_tensor(d["K"], device=device)
    if kind == "cost":
        Bt, Qt = ca.assemble_batch(dev(d["pts_2d"]), None, dev(d["pts_3d"]), None, K, device=device)
        Qt = Qt.reshape(batch, 45).clone()
        diag = [k * 9 - k * (k - 1) // 2 for k in range(9)]  # packed index of (k, k): the upper triangle row by row
        tr = Qt[:, diag].sum(dim=1)
        for p, k in INDEFINITE.items():
            Qt[p, diag[k]] -= 0.5 * tr[p]
        Qt[NAN_AT[0], NAN_AT[1]] = float("nan")
        res = ca.solve_cost_batch(Qt, Bt, want_Z=True, device=device, **opts)
    else:
        res = ca.pnp_batch(dev(d["pts_2d"]), dev(d["pts_3d"]), K, want_Z=True, **opts)
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


def keys():
    """every name the fixture holds"""
    want = set()
    for name in CASES:
        want |= set(stored(name, {k: np.zeros(1) for k in INTS + FLOATS}))
        if noisy(name):
            want.add(f"{name}__sigma")
    return want


def main():
    import torch

    sys.path.insert(0, ROOT)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    device = torch.device("cuda:0")
    keep = {}
    for name in CASES:
        first = CASES[name][5]
        sigma = None
        if noisy(name):
            for s in NOISE_LEVELS:
                it = run_case(name, device, s)["iters"]
                share = float((it > first).mean())
                print(name, "sigma", s, "share of problems past the first attempt", round(share, 3), flush=True)
                if share >= NOISY_SHARE:
                    sigma = s
                    break
            assert sigma is not None, f"{name}: no noise level of {NOISE_LEVELS} leaves {NOISY_SHARE:.0%} of the problems open after the first attempt"
            keep[f"{name}__sigma"] = np.float64(sigma)
        a, b = run_case(name, device, sigma), run_case(name, device, sigma)
        for k in a:  # the record must be a function of the inputs alone
            assert a[k].tobytes() == b[k].tobytes(), f"{name}__{k}: two runs of the same library differ"
        if noisy(name):
            assert (a["iters"] > first).mean() >= NOISY_SHARE, name
        if CASES[name][0] == "cost":
            assert (a["status"] != ST_CERTIFIED).any(), f"{name}: every problem certified"
        keep.update(stored(name, a))
        print(name, "status", np.bincount(a["status"], minlength=5).tolist(), "iters", np.bincount(a["iters"]).nonzero()[0].tolist(), flush=True)
    assert set(keep) == keys()
    np.savez_compressed(path, **keep)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
