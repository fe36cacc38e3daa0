"""The library of adaptive and guided RANSAC over points and lines (libcvxpnpl_amd_ransac_pnpl_adaptive.so,
include/cvxpnpl_amd_ransac_pnpl_adaptive.h): it builds by cross-compilation, exports what its header declares and
nothing else, rejects bad arguments before it touches a device, keeps its kernels free of scratch and spills
(tests/golden/ransac_pnpl_adaptive_kernel_resources.json) and leaves the other ten libraries alone; the numpy restatement of the guided
union draw and of the round replay (tests/ransac_pnpl_adaptive_reference.py); and the host-side validation of
ransac_pnpl_batch(confidence=..., round_hyp=..., quality=..., line_quality=..., pool_full=...).  No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_pnpl_adaptive_reference import guided_union_sets, packed_order, replay, union_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_pnpl_adaptive_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxnla::sample_assemble_active_kernel", "cvxnla::score_pnpl_active_kernel", "cvxnla::update_pnpl_active_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_pnpl_adaptive()
    assert os.path.exists(build.RANSAC_PNPL_ADAPTIVE_OUT)
    return _lib.ransac_pnpl_adaptive_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_pnpl_adaptive.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_PNPL_ADAPTIVE_EXPORTS), declared ^ set(_lib.RANSAC_PNPL_ADAPTIVE_EXPORTS)
    assert declared == {"cvxpnpl_ransac_pnpl_adaptive_" + n for n in ("sample_assemble", "score", "update", "last_error")}
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_PNPL_ADAPTIVE_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library():
    from cvxpnpl_amd import build as b

    assert b.ransac_pnpl_adaptive_compile_cmd("x")[:-1] == b.ransac_compile_cmd("x")[:-1]


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_pnpl_adaptive_last_error
    nan, z = float("nan"), None

    def sample(F=2, A=2, act=p, h0=0, Hr=8, cap=8, pf=0, offp=p, npts=10, offl=p, nln=6, seeds=p, order=None, p2=p, p3=p, l2=p, l3=p, K=p, per=0,
               idx=None, Q=p, B=p):
        return G.cvxpnpl_ransac_pnpl_adaptive_sample_assemble(F, A, act, h0, Hr, cap, pf, offp, npts, offl, nln, seeds, order, p2, p3, l2, l3, K, per,
                                                              idx, Q, B, None)

    assert sample(offp=None) == -1
    assert b"cvxpnpl_ransac_pnpl_adaptive_sample_assemble: bad arguments" in err() and b"offsets" in err()
    assert sample(offl=None) == -1 and sample(act=None) == -1 and b"d_active" in err()
    assert sample(F=-1) == -1 and sample(A=-1) == -1 and sample(npts=-1) == -1 and sample(nln=-1) == -1       # negative sizes
    assert b"negative size" in err()
    assert sample(F=2**31) == -1 and sample(A=2**31) == -1
    assert sample(Hr=-8) == -1 and sample(h0=-1) == -1 and sample(cap=-1, Hr=0) == -1
    assert sample(h0=4, Hr=8, cap=11) == -1 and b"exceeds cap" in err()                                       # hyp0 + Hr > cap
    assert sample(h0=2**31 - 1, Hr=2**31 - 1, cap=2**31 - 1) == -1 and b"exceeds cap" in err()                # ... without wrapping
    assert sample(pf=-1) == -1 and b"pool_full" in err()
    assert sample(pf=1, order=None) == -1 and b"d_order" in err()                                             # a ranking is needed before pool_full
    assert sample(per=2) == -1 and sample(per=-1) == -1 and b"K_per_scene" in err()
    assert sample(seeds=None) == -1 and sample(K=None) == -1 and sample(Q=None) == -1 and sample(B=None) == -1
    assert sample(p2=None) == -1 and sample(p3=None) == -1 and sample(l2=None) == -1 and sample(l3=None) == -1

    def score(F=2, A=2, act=p, Hr=8, offp=p, npts=10, offl=p, nln=6, R=p, t=p, st=None, um=5, K=p, per=0, p2=p, p3=p, l2=p, l3=p, th=2.0, cnt=p):
        return G.cvxpnpl_ransac_pnpl_adaptive_score(F, A, act, Hr, offp, npts, offl, nln, R, t, st, um, K, per, p2, p3, l2, l3, th, cnt, None)

    assert score(R=None) == -1
    assert b"cvxpnpl_ransac_pnpl_adaptive_score: bad arguments" in err()
    assert score(act=None) == -1 and score(offp=None) == -1 and score(offl=None) == -1 and score(t=None) == -1 and score(K=None) == -1
    assert score(cnt=None) == -1 and score(per=2) == -1 and score(Hr=-1) == -1 and score(npts=-1) == -1 and score(nln=-1) == -1 and score(l3=None) == -1
    assert score(th=nan) == -1 and b"thresh" in err() and score(th=-1.0) == -1 and b"thresh" in err()

    def update(F=2, A=2, act=p, h0=0, Hr=8, cap=8, conf=0.99, offp=p, npts=10, offl=p, nln=6, cnt=p, R=p, t=p, st=p, K=p, per=0, p2=p, p3=p, l2=p,
               l3=p, th=2.0, oR=p, ot=p, head=p, best=p, mp=p, ml=p, used=p, done=p):
        return G.cvxpnpl_ransac_pnpl_adaptive_update(F, A, act, h0, Hr, cap, conf, offp, npts, offl, nln, cnt, R, t, st, K, per, p2, p3, l2, l3, th, oR,
                                                     ot, head, best, mp, ml, used, done, None)

    assert update(conf=nan) == -1
    assert b"cvxpnpl_ransac_pnpl_adaptive_update: bad arguments" in err() and b"confidence" in err()
    for conf in (0.0, 1.0, -0.5, 1.5, float("inf"), -float("inf")):                                           # confidence outside (0, 1)
        assert update(conf=conf) == -1 and b"confidence" in err(), conf
    assert update(Hr=-8) == -1 and update(h0=-1) == -1 and update(cap=-1, Hr=0) == -1 and update(h0=4, Hr=8, cap=11) == -1
    assert update(h0=2**31 - 1, Hr=2**31 - 1, cap=2**31 - 1) == -1
    assert update(Hr=0) == -1 and b"at least one hypothesis" in err()                                         # a round without hypotheses
    assert update(act=None) == -1 and update(offp=None) == -1 and update(cnt=None) == -1 and update(st=None) == -1 and update(K=None) == -1
    assert update(head=None) == -1 and update(best=None) == -1 and update(mp=None) == -1 and update(ml=None) == -1 and update(used=None) == -1
    assert update(done=None) == -1 and update(oR=None) == -1 and update(ot=None) == -1 and update(per=3) == -1 and update(F=-2) == -1
    assert update(th=nan) == -1 and update(th=-0.5) == -1 and update(npts=-1) == -1 and update(nln=-1) == -1

    # a zero-size call is a no-op whatever the pointers
    for kw in (dict(F=0, npts=0, nln=0), dict(A=0)):
        assert sample(act=z, offp=z, offl=z, seeds=z, p2=z, p3=z, l2=z, l3=z, K=z, Q=z, B=z, **kw) == 0
        assert score(act=z, offp=z, offl=z, R=z, t=z, K=z, p2=z, p3=z, l2=z, l3=z, cnt=z, **kw) == 0
        assert update(act=z, offp=z, offl=z, cnt=z, R=z, t=z, st=z, K=z, p2=z, p3=z, l2=z, l3=z, oR=z, ot=z, head=z, best=z, mp=z, ml=z, used=z,
                      done=z, **kw) == 0
    assert sample(Hr=0, seeds=z, K=z, Q=z, B=z) == 0 and score(Hr=0, R=z, t=z, K=z, cnt=z) == 0
    # ... but not one with a bad size or budget beside the zero
    assert sample(A=0, pf=-1) == -1 and sample(A=0, npts=-1) == -1 and update(A=0, conf=nan) == -1 and update(A=0, h0=5, Hr=8, cap=8) == -1


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

    assert os.path.exists(b.RANSAC_PNPL_ADAPTIVE_RESOURCES)
    assert os.path.getmtime(b.RANSAC_PNPL_ADAPTIVE_RESOURCES) >= os.path.getmtime(b.RANSAC_PNPL_ADAPTIVE_OUT) - 1
    table = b.kernel_resources(b.RANSAC_PNPL_ADAPTIVE_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)
    assert all(g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0 for g in golden.values())
    assert golden["cvxnla::score_pnpl_active_kernel"]["lds"] == 512 * 5 * 8   # LDS is the scoring tile's ...
    assert all(g["lds"] <= 64 for k, g in golden.items() if "score_pnpl_active" not in k)   # ... and a few words for the cross-wave reductions


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the other ten, and the tables of the four RANSAC
    libraries it borrows from still hold -- the third's, the fourth's (after its device functions moved into ransac_pnpl_common.h: the
    same kernel set), the ninth's and the tenth's."""
    from cvxpnpl_amd import build as b

    b.build()
    others = {"solver": b.RESOURCES, "grad": b.GRAD_RESOURCES, "ransac": b.RANSAC_RESOURCES, "ransac_pnpl": b.RANSAC_PNPL_RESOURCES,
              "refine": b.REFINE_RESOURCES, "refine_grad": b.REFINE_GRAD_RESOURCES, "refine_robust": b.REFINE_ROBUST_RESOURCES,
              "refine_robust_grad": b.REFINE_ROBUST_GRAD_RESOURCES, "ransac_adaptive": b.RANSAC_ADAPTIVE_RESOURCES,
              "ransac_guided": b.RANSAC_GUIDED_RESOURCES}
    tables = {lib: b.kernel_resources(path) for lib, path in others.items()}
    short = [k.split("::")[-1] for k in KERNELS]
    for lib, table in tables.items():
        assert table, lib
        assert not [k for k in table if "cvxnla::" in k or any(n in k for n in short)], lib
    for lib, name in (("ransac", "ransac_kernel_resources.json"), ("ransac_pnpl", "ransac_pnpl_kernel_resources.json"),
                      ("ransac_adaptive", "ransac_adaptive_kernel_resources.json"), ("ransac_guided", "ransac_guided_kernel_resources.json")):
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert set(tables[lib]) == set(golden), (lib, set(tables[lib]) ^ set(golden))
        problems = _compare(tables[lib], golden)
        assert not problems, "\n".join(problems)


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------------
def test_the_reference_of_the_guided_union_draw():
    from cvxpnpl_amd import synth

    from ransac_guided_reference import pools

    P, L, seed, H = 6, 5, 77, 40
    qp, ql = np.array([0.1, 0.9, 0.3, np.nan, 0.9, 0.2]), np.array([0.95, 0.0, 0.9, 0.5, -1.0])
    order = union_rank(qp, ql)
    assert list(order) == [6, 1, 4, 8, 9, 2, 5, 0, 7, 10, 3]          # one scale: line 0 first, ties by union index, the NaN last
    sets = guided_union_sets(H, P, L, order, 20, seed)
    assert sets.shape == (H, 4) and sorted(sets[0]) == [1, 4, 6, 8]   # hypothesis 0 draws the four best: two points, two lines
    uni = synth.philox_minimal_sets(H, P + L, 4, seed)
    assert np.array_equal(sets[20:], uni[20:])                        # from pool_full on: the uniform draw, not read through order
    n = pools(np.arange(20), P + L, 20)
    for h in range(20):                                               # before: four distinct members of the n(h) best
        assert len(set(sets[h])) == 4 and set(sets[h]) <= set(order[:n[h]].tolist()), h
    assert np.array_equal(guided_union_sets(H, P, L, order, 0, seed), uni)                     # pool_full = 0: the uniform sampler
    assert np.array_equal(guided_union_sets(12, P, L, order, 20, seed, h0=14), sets[14:26])    # a round is a slice, also across pool_full
    assert np.array_equal(guided_union_sets(H, 0, P + L, order, 20, seed), sets)               # the draw does not know what an index is
    assert list(packed_order([order, order[:4] % 4], [(P, L), (1, 3)])[-4:]) == list(order[:4] % 4)


def test_the_reference_replay_counts_points_and_lines():
    """The stopping rule runs on M_f = P_f + L_f: the same counts stop a (2, 2) scene at once and leave a (6, 4) scene running."""
    from ransac_adaptive_reference import needed

    shapes = [(2, 2), (6, 4), (0, 10), (10, 0)]
    counts = np.zeros((4, 20), dtype=np.int64)
    status = np.zeros((4, 20), dtype=np.int64)
    counts[0, 3] = 4                     # all of (2, 2) in round 0: N = 0
    counts[1, 3] = 4                     # 4 of 10: far from enough
    counts[2, 2] = counts[2, 9] = 8      # a tie across rounds: index 2 stays
    counts[3, 17] = 9                    # found in the last, short round
    out = replay(counts, status, shapes, 0.99, 8, 20)
    assert [list(a) for a in out["active"]] == [[0, 1, 2, 3], [1, 2, 3], [1, 3]]
    assert list(out["hyp_used"]) == [8, 20, 16, 20] and list(out["winner"]) == [3, 3, 2, 17] and list(out["best"]) == [4, 4, 8, 9]
    assert 8 < needed(8, 10, 0.99) < 16 and needed(4, 4, 0.99) == 0.0 and needed(4, 10, 0.99) > 20


# ---- host validation of the keywords ------------------------------------------------------------------------------------------------------
def _scene(p, l, rs):
    return rs.random_sample((p, 2)), rs.random_sample((l, 2, 2)), rs.random_sample((p, 3)), rs.random_sample((l, 2, 3))


def test_keywords_are_validated_on_the_host():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import inspect

    from cvxpnpl_amd.ransac import ransac_pnl, ransac_pnl_batch, ransac_pnpl, ransac_pnpl_batch

    sig = inspect.signature(ransac_pnpl_batch).parameters
    assert sig["confidence"].default is None and sig["round_hyp"].default == 64
    assert sig["quality"].default is None and sig["line_quality"].default is None and sig["pool_full"].default is None
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a, b = _scene(6, 3, rs), _scene(2, 5, rs)
    lists = tuple([x, y] for x, y in zip(a, b)) + (K,)
    qa, qb, la, lb = rs.random_sample(6), rs.random_sample(2), rs.random_sample(3), rs.random_sample(5)
    for bad in (0.0, 1.0, -0.1, 1.01, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="confidence"):
            ransac_pnpl_batch(*lists, confidence=bad)
    for bad in (0, -1, -64):
        with pytest.raises(ValueError, match="round_hyp"):
            ransac_pnpl_batch(*lists, confidence=0.99, round_hyp=bad)
    with pytest.raises(ValueError, match="n_hyp"):
        ransac_pnpl_batch(*lists, confidence=0.99, n_hyp=0)
    with pytest.raises(ValueError, match="n_hyp"):
        ransac_pnpl_batch(*lists, quality=[qa, qb], line_quality=[la, lb], n_hyp=0)
    with pytest.raises(ValueError, match="pool_full given without quality"):
        ransac_pnpl_batch(*lists, pool_full=4)
    for bad in (-1, 1.5, "4", True, 2**31):
        with pytest.raises(ValueError, match="pool_full"):
            ransac_pnpl_batch(*lists, quality=[qa, qb], line_quality=[la, lb], pool_full=bad)
    with pytest.raises(ValueError, match="line_quality is missing"):      # lines present, no line quality
        ransac_pnpl_batch(*lists, quality=[qa, qb])
    with pytest.raises(ValueError, match=r"points, quality is missing"):  # ... and the reverse
        ransac_pnpl_batch(*lists, line_quality=[la, lb])
    with pytest.raises(ValueError, match="hold no lines"):                # a quality for a kind the scenes do not hold
        ransac_pnpl_batch([a[0], a[0]], None, [a[2], a[2]], None, K, quality=[qa, qa], line_quality=[la, la])
    with pytest.raises(ValueError, match="hold no points"):
        ransac_pnl_batch([b[1], b[1]], [b[3], b[3]], K, quality=[qb, qb], line_quality=[lb, lb])
    with pytest.raises(ValueError, match="scene 1: quality"):             # a wrong length
        ransac_pnpl_batch(*lists, quality=[qa, qb[:1]], line_quality=[la, lb])
    with pytest.raises(ValueError, match="scene 0: line_quality"):
        ransac_pnpl_batch(*lists, quality=[qa, qb], line_quality=[la[:2], lb])
    with pytest.raises(ValueError, match="line_quality"):                 # a wrong shape
        ransac_pnpl_batch(*lists, quality=[qa, qb], line_quality=[la, lb.reshape(5, 1)])
    with pytest.raises(ValueError, match="quality for 1 scenes"):         # a scene's quality missing
        ransac_pnpl_batch(*lists, quality=[qa], line_quality=[la, lb])
    with pytest.raises(ValueError, match="quality"):                      # packed where a list is due
        ransac_pnpl_batch(*lists, quality=np.concatenate([qa, qb]), line_quality=[la, lb])
    packed = tuple(np.concatenate([x, y]) for x, y in zip(a, b)) + (K,)
    with pytest.raises(ValueError, match="line_quality"):                 # packed: the wrong total
        ransac_pnpl_batch(*packed, sizes=[6, 2], line_sizes=[3, 5], quality=np.concatenate([qa, qb]), line_quality=np.concatenate([la, lb])[:7])
    with pytest.raises(ValueError, match="real numbers"):
        ransac_pnpl_batch(*lists, quality=[qa.astype(np.complex128), qb], line_quality=[la, lb])
    with pytest.raises(ValueError, match="needs 4"):                      # the scene set is still validated first
        ransac_pnpl_batch([a[0], b[0]], [a[1], b[1][:1]], [a[2], b[2]], [a[3], b[3][:1]], K, confidence=2.0, quality=[qa], pool_full=-1)
    with pytest.raises(ValueError, match="confidence"):                   # both sets of keywords are checked
        ransac_pnpl_batch(*lists, quality=[qa, qb], line_quality=[la, lb], confidence=1.0)
    # the wrappers pass the keywords through
    with pytest.raises(ValueError, match="confidence"):
        ransac_pnl_batch([b[1], b[1]], [b[3], b[3]], K, confidence=0.0)
    with pytest.raises(ValueError, match="line_quality is missing"):
        ransac_pnpl(*a, K, quality=qa)
    with pytest.raises(ValueError, match="round_hyp"):
        ransac_pnpl(*a, K, confidence=0.9, round_hyp=0)
    with pytest.raises(ValueError, match="scene 0: line_quality"):
        ransac_pnl(b[1], b[3], K, line_quality=lb[:4])
