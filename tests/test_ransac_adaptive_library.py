"""The library of adaptive RANSAC (libcvxpnpl_amd_ransac_adaptive.so, include/cvxpnpl_amd_ransac_adaptive.h): it
builds by cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps
its kernels free of scratch and spills (tests/golden/ransac_adaptive_kernel_resources.json) and leaves the other libraries alone; its
stopping rule on the host against the numpy reference (tests/ransac_adaptive_reference.py); and the host-side validation of
ransac_pnp_batch(confidence=..., round_hyp=...).  No GPU needed."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_adaptive_reference import needed, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_adaptive_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxna::adaptive_init_kernel", "cvxna::sample_active_kernel", "cvxna::score_active_kernel", "cvxna::round_update_kernel",
           "cvxna::compact_active_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_adaptive()
    assert os.path.exists(build.RANSAC_ADAPTIVE_OUT)
    return _lib.ransac_adaptive_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_adaptive.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_ADAPTIVE_EXPORTS), declared ^ set(_lib.RANSAC_ADAPTIVE_EXPORTS)
    assert all(name.startswith("cvxpnpl_ransac_adaptive_") for name in declared)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_ADAPTIVE_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library():
    from cvxpnpl_amd import build as b

    assert b.ransac_adaptive_compile_cmd("x")[:-1] == b.ransac_compile_cmd("x")[:-1]


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_adaptive_last_error
    nan, z = float("nan"), None

    def init(F=2, act=p, n=p, head=p, best=p, used=p):
        return G.cvxpnpl_ransac_adaptive_init(F, act, n, head, best, used, None)

    assert init(act=None) == -1
    assert b"cvxpnpl_ransac_adaptive_init: bad arguments" in err()
    assert init(n=None) == -1 and init(head=None) == -1 and init(best=None) == -1 and init(used=None) == -1 and init(F=-1) == -1
    assert init(F=2**31) == -1

    def sample(F=2, A=2, act=p, h0=0, Hr=8, cap=8, off=p, tot=10, seeds=p, s2=p, s3=p, K=None, idx=None, p2=p, p3=p, Kh=None):
        return G.cvxpnpl_ransac_adaptive_sample(F, A, act, h0, Hr, cap, off, tot, seeds, s2, s3, K, idx, p2, p3, Kh, None)

    assert sample(off=None) == -1
    assert b"cvxpnpl_ransac_adaptive_sample: bad arguments" in err() and b"d_offsets" in err()
    assert sample(act=None) == -1 and b"d_active" in err()
    assert sample(F=-1) == -1 and sample(A=-1) == -1 and sample(tot=-1) == -1
    assert sample(Hr=-8) == -1 and sample(h0=-1) == -1 and sample(cap=-1, Hr=0) == -1          # round_hyp, hyp0 or the cap negative
    assert sample(h0=4, Hr=8, cap=11) == -1 and b"exceeds cap" in err()                         # hyp0 + Hr > cap
    assert sample(h0=2**31 - 1, Hr=2**31 - 1, cap=2**31 - 1) == -1                              # ... without wrapping
    assert sample(seeds=None) == -1 and sample(p2=None) == -1 and sample(p3=None) == -1 and sample(s2=None) == -1
    assert sample(K=p) == -1 and sample(Kh=p) == -1                                             # K and K_hyp go together

    def score(F=2, A=2, act=p, Hr=8, off=p, tot=10, R=p, t=p, st=None, um=5, K=p, per=0, s2=p, s3=p, th=2.0, cnt=p):
        return G.cvxpnpl_ransac_adaptive_score(F, A, act, Hr, off, tot, R, t, st, um, K, per, s2, s3, th, cnt, None)

    assert score(R=None) == -1
    assert b"cvxpnpl_ransac_adaptive_score: bad arguments" in err()
    assert score(act=None) == -1 and score(off=None) == -1 and score(t=None) == -1 and score(K=None) == -1 and score(cnt=None) == -1
    assert score(per=2) == -1 and score(th=nan) == -1 and score(th=-1.0) == -1 and score(Hr=-1) == -1 and score(tot=-1) == -1 and score(s3=None) == -1

    def update(F=2, A=2, act=p, h0=0, Hr=8, cap=8, conf=0.99, off=p, tot=10, cnt=p, R=p, t=p, st=p, K=p, per=0, s2=p, s3=p, th=2.0, oR=p, ot=p,
               head=p, best=p, mask=p, used=p, done=p):
        return G.cvxpnpl_ransac_adaptive_update(F, A, act, h0, Hr, cap, conf, off, tot, cnt, R, t, st, K, per, s2, s3, th, oR, ot, head, best, mask,
                                                used, done, None)

    assert update(conf=nan) == -1
    assert b"cvxpnpl_ransac_adaptive_update: bad arguments" in err() and b"confidence" in err()
    for conf in (0.0, 1.0, -0.5, 1.5, float("inf"), -float("inf")):                             # confidence outside (0, 1)
        assert update(conf=conf) == -1, conf
    assert update(Hr=-8) == -1 and update(h0=-1) == -1 and update(cap=-1, Hr=0) == -1 and update(h0=4, Hr=8, cap=11) == -1
    assert update(Hr=0) == -1                                                                   # a round without hypotheses
    assert update(act=None) == -1 and update(off=None) == -1 and update(cnt=None) == -1 and update(st=None) == -1 and update(K=None) == -1
    assert update(head=None) == -1 and update(best=None) == -1 and update(mask=None) == -1 and update(used=None) == -1 and update(done=None) == -1
    assert update(oR=None) == -1 and update(ot=None) == -1 and update(per=3) == -1 and update(th=nan) == -1 and update(F=-2) == -1

    def compact(F=2, A=2, act=p, done=p, nxt=C.c_void_p(16), n=p):
        return G.cvxpnpl_ransac_adaptive_compact(F, A, act, done, nxt, n, None)

    assert compact(act=None) == -1
    assert b"cvxpnpl_ransac_adaptive_compact: bad arguments" in err()
    assert compact(done=None) == -1 and compact(nxt=None) == -1 and compact(n=None) == -1 and compact(A=-1) == -1 and compact(F=-1) == -1
    assert compact(nxt=p) == -1 and b"must not be d_active" in err()                            # in place

    # a zero-size call is a no-op whatever the pointers
    assert init(F=0, act=z, n=z, head=z, best=z, used=z) == 0
    for kw in (dict(F=0, tot=0), dict(A=0)):
        assert sample(act=z, off=z, seeds=z, s2=z, s3=z, p2=z, p3=z, **kw) == 0
        assert score(act=z, off=z, R=z, t=z, K=z, s2=z, s3=z, cnt=z, **kw) == 0
        assert update(act=z, off=z, cnt=z, R=z, t=z, st=z, K=z, s2=z, s3=z, oR=z, ot=z, head=z, best=z, mask=z, used=z, done=z, **kw) == 0
    assert compact(F=0, act=z, done=z, nxt=z, n=z) == 0 and compact(A=0, act=z, done=z, nxt=z, n=z) == 0
    assert sample(Hr=0, seeds=z, p2=z, p3=z) == 0 and score(Hr=0, R=z, t=z, K=z, cnt=z) == 0


def _compare(table, golden):
    problems = []
    for name, g in golden.items():
        r = table[name]
        for k in ("occupancy", "lds", "scratch", "sgpr_spill", "vgpr_spill"):
            if r[k] != g[k]:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]}")
        for k in ("vgpr", "agpr"):
            if r[k] > g[k] + REG_SLACK:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]} (+{REG_SLACK} allowed)")
        if g["scratch"] or g["vgpr_spill"] or g["sgpr_spill"]:
            problems.append(f"{name}: the table itself admits scratch or spills")
    return problems


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.RANSAC_ADAPTIVE_RESOURCES) and os.path.getmtime(b.RANSAC_ADAPTIVE_RESOURCES) >= os.path.getmtime(b.RANSAC_ADAPTIVE_OUT) - 1
    table = b.kernel_resources(b.RANSAC_ADAPTIVE_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)
    assert golden["cvxna::score_active_kernel"]["lds"] == 512 * 5 * 8   # LDS is the scoring tile's ...
    assert all(g["lds"] <= 64 for k, g in golden.items() if "score_active" not in k)   # ... and a few words for the cross-wave reductions


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the other eight, and the solver's, the gradient's
    and the two RANSAC libraries' tables still hold (the third library's after block_inliers moved into ransac_common.h)."""
    import test_kernel_resources as tkr
    from cvxpnpl_amd import build as b

    b.build()
    others = {"solver": b.RESOURCES, "grad": b.GRAD_RESOURCES, "ransac": b.RANSAC_RESOURCES, "ransac_pnpl": b.RANSAC_PNPL_RESOURCES,
              "refine": b.REFINE_RESOURCES, "refine_grad": b.REFINE_GRAD_RESOURCES, "refine_robust": b.REFINE_ROBUST_RESOURCES,
              "refine_robust_grad": b.REFINE_ROBUST_GRAD_RESOURCES}
    tables = {lib: b.kernel_resources(path) for lib, path in others.items()}
    short = [k.split("::")[-1] for k in KERNELS]
    for lib, table in tables.items():
        assert table, lib
        assert not [k for k in table if "cvxna::" in k or any(n in k for n in short)], lib
    problems = tkr._compare(tables["solver"], json.load(open(tkr.GOLDEN)))
    assert not problems, "\n".join(problems)
    for lib, name in (("grad", "grad_kernel_resources.json"), ("ransac", "ransac_kernel_resources.json"), ("ransac_pnpl", "ransac_pnpl_kernel_resources.json")):
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert set(tables[lib]) == set(golden), (lib, set(tables[lib]) ^ set(golden))
        problems = _compare(tables[lib], golden)
        assert not problems, "\n".join(problems)


def test_the_rule_on_the_host_equals_the_reference(G):
    from cvxpnpl_amd.ransac import needed_hypotheses

    host = G.cvxpnpl_ransac_adaptive_needed_host
    worst = 0.0
    for M in (4, 5, 64, 100, 700, 10**4):
        for p in (0.5, 0.99, 0.999999):
            prev = math.inf
            for I in range(0, M + 1):
                got, ref = host(I, M, p), needed(I, M, p)
                if I < 4:
                    assert got == math.inf and ref == math.inf, (I, M, p, got)
                elif I == M:
                    assert got == 0.0 and ref == 0.0, (I, M, p, got)
                else:
                    assert math.isfinite(got) and got > 0.0, (I, M, p, got)
                    rel = abs(got - ref) / abs(ref)
                    worst = max(worst, rel)
                    assert rel <= 1e-12, (I, M, p, got, ref)
                assert got <= prev, (I, M, p, got, prev)    # non-increasing in I
                prev = got
    print(f"needed_host against the reference: worst relative difference {worst:.2e}")
    assert 17.0 < needed(70, 100, 0.99) < 18.0 and 17.0 < host(70, 100, 0.99) < 18.0   # the README scene: 18 hypotheses
    assert needed_hypotheses(70, 100, 0.99) == host(70, 100, 0.99)
    assert 76.0 < needed(50, 100, 0.99) < 77.0                                          # 50 % outliers: q = 0.0587 without replacement, 77 hypotheses
    for bad in (0.0, 1.0, -1.0, 2.0, float("nan")):
        assert math.isnan(host(70, 100, bad)), bad


def test_the_reference_replay():
    """simulate on hand-made counts: a first-round stop, a tie that a later round does not take, a run to the cap, a short last round."""
    counts = np.zeros((4, 20), dtype=np.int64)
    status = np.zeros((4, 20), dtype=np.int64)
    sizes = [10, 10, 10, 10]
    counts[0, 3] = 10                    # all inliers in round 0: N = 0
    counts[1, 2] = counts[1, 9] = 8      # a tie across rounds: index 2 stays
    counts[2, 17] = 9                    # found in the last, short round
    status[3, ::2] = 2                   # scene 3: nothing but zeros, half of them uncertified
    out = simulate(counts, status, sizes, 0.99, 8, 20)
    assert [list(a) for a in out["active"]] == [[0, 1, 2, 3], [1, 2, 3], [2, 3]]
    assert list(out["hyp_used"]) == [8, 16, 20, 20] and list(out["winner"]) == [3, 2, 17, 0] and list(out["best"]) == [10, 8, 9, 0]
    assert list(out["certified"]) == [8, 16, 20, 10]
    assert 8 < needed(8, 10, 0.99) < 16


def _scene(m, rs):
    return rs.random_sample((m, 2)), rs.random_sample((m, 3))


def test_adaptive_keywords_are_validated_on_the_host():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import inspect

    from cvxpnpl_amd.ransac import ransac_pnp_batch

    sig = inspect.signature(ransac_pnp_batch).parameters
    assert sig["confidence"].default is None and sig["round_hyp"].default == 64
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3 = _scene(10, rs)
    b2, b3 = _scene(7, rs)
    for bad in (0.0, 1.0, -0.1, 1.01, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="confidence"):
            ransac_pnp_batch([a2, b2], [a3, b3], K, confidence=bad)
    for bad in (0, -1, -64):
        with pytest.raises(ValueError, match="round_hyp"):
            ransac_pnp_batch([a2, b2], [a3, b3], K, confidence=0.99, round_hyp=bad)
    with pytest.raises(ValueError, match="n_hyp"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, confidence=0.99, n_hyp=0)
    with pytest.raises(ValueError, match="needs 4"):          # the scene set is still validated first
        ransac_pnp_batch([a2, b2[:3]], [a3, b3[:3]], K, confidence=0.99)
