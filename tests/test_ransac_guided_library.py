"""The library of guided RANSAC (libcvxpnpl_amd_ransac_guided.so, include/cvxpnpl_amd_ransac_guided.h): it builds by
cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels
free of scratch and spills (tests/golden/ransac_guided_kernel_resources.json) and leaves the other libraries alone; its pool rule and
its ranking on the host against the numpy reference (tests/ransac_guided_reference.py), exactly; and the host-side validation of
ransac_pnp_batch(quality=..., pool_full=...).  No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_guided_reference import first_all_inlier, guided_sets, planted_quality, pool, pools, quality_patterns, rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_guided_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxng::rank_quality_kernel", "cvxng::sample_guided_kernel", "cvxng::sample_guided_active_kernel")
SIZES = [4, 4, 5, 63, 64, 65, 100, 255, 256, 257, 511, 512, 513, 700]   # the scenes of tests/test_ransac_guided_gpu.py


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_guided()
    assert os.path.exists(build.RANSAC_GUIDED_OUT)
    return _lib.ransac_guided_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_guided.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_GUIDED_EXPORTS), declared ^ set(_lib.RANSAC_GUIDED_EXPORTS)
    assert declared == {"cvxpnpl_ransac_guided_" + n for n in ("rank", "sample", "sample_active", "rank_host", "pool_host", "last_error")}
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_GUIDED_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library():
    from cvxpnpl_amd import build as b

    assert b.ransac_guided_compile_cmd("x")[:-1] == b.ransac_compile_cmd("x")[:-1]
    assert b.ransac_guided_compile_cmd("x")[-1] == b.RANSAC_GUIDED_SRC and b.RANSAC_GUIDED_RESOURCES != b.RANSAC_ADAPTIVE_RESOURCES


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_guided_last_error
    z = None

    def rnk(F=2, off=p, tot=10, mx=6, q=p, order=p):
        return G.cvxpnpl_ransac_guided_rank(F, off, tot, mx, q, order, None)

    assert rnk(off=None) == -1
    assert b"cvxpnpl_ransac_guided_rank: bad arguments" in err() and b"d_offsets" in err()
    assert rnk(q=None) == -1 and b"d_quality" in err()
    assert rnk(order=None) == -1 and b"d_order" in err()
    assert rnk(F=-1) == -1 and b"n_scenes" in err()
    assert rnk(tot=-1) == -1 and b"n_total" in err()
    assert rnk(mx=-1) == -1 and b"max_corr" in err()
    assert rnk(F=2**31) == -1

    def sample(F=2, H=8, pf=8, off=p, tot=10, seeds=p, order=p, s2=p, s3=p, K=None, idx=None, p2=p, p3=p, Kh=None):
        return G.cvxpnpl_ransac_guided_sample(F, H, pf, off, tot, seeds, order, s2, s3, K, idx, p2, p3, Kh, None)

    assert sample(off=None) == -1
    assert b"cvxpnpl_ransac_guided_sample: bad arguments" in err() and b"d_offsets" in err()
    assert sample(pf=-1) == -1 and b"pool_full" in err()
    assert sample(H=-1) == -1 and b"n_hyp" in err()
    assert sample(F=-1) == -1 and b"n_scenes" in err()
    assert sample(tot=-1) == -1 and b"n_total" in err()
    assert sample(seeds=None) == -1 and b"d_seeds" in err()
    assert sample(order=None) == -1 and b"d_order" in err()
    assert sample(p2=None) == -1 and b"d_pts_2d" in err()
    assert sample(p3=None) == -1 and sample(s2=None) == -1 and sample(s3=None) == -1 and b"d_scene_2d" in err()
    assert sample(K=p) == -1 and b"d_K_hyp" in err()                                            # K and K_hyp go together
    assert sample(Kh=p) == -1

    def active(F=2, A=2, act=p, h0=0, Hr=8, cap=8, pf=8, off=p, tot=10, seeds=p, order=p, s2=p, s3=p, K=None, idx=None, p2=p, p3=p, Kh=None):
        return G.cvxpnpl_ransac_guided_sample_active(F, A, act, h0, Hr, cap, pf, off, tot, seeds, order, s2, s3, K, idx, p2, p3, Kh, None)

    assert active(act=None) == -1
    assert b"cvxpnpl_ransac_guided_sample_active: bad arguments" in err() and b"d_active" in err()
    assert active(off=None) == -1 and b"d_offsets" in err()
    assert active(pf=-1) == -1 and b"pool_full" in err()
    assert active(h0=-1) == -1 and b"hyp0" in err()
    assert active(Hr=-8) == -1 and b"n_round" in err()
    assert active(cap=-1, Hr=0) == -1 and b"cap" in err()
    assert active(tot=-1) == -1 and b"n_total" in err()
    assert active(F=-1) == -1 and active(A=-1) == -1 and b"n_active" in err()
    assert active(h0=4, Hr=8, cap=11) == -1 and b"exceeds cap" in err()                         # hyp0 + n_round > cap
    assert active(h0=2**31 - 1, Hr=2**31 - 1, cap=2**31 - 1) == -1 and b"exceeds cap" in err()  # ... without wrapping
    assert active(seeds=None) == -1 and active(order=None) == -1 and active(p2=None) == -1 and active(p3=None) == -1 and active(s2=None) == -1
    assert active(K=p) == -1 and active(Kh=p) == -1

    def rank_host(F=2, off=p, tot=10, q=p, order=p):
        return G.cvxpnpl_ransac_guided_rank_host(F, off, tot, q, order, 1)

    assert rank_host(off=None) == -1 and b"cvxpnpl_ransac_guided_rank_host: bad arguments" in err() and b"offsets" in err()
    assert rank_host(q=None) == -1 and b"quality" in err()
    assert rank_host(order=None) == -1 and b"order" in err()
    assert rank_host(F=-1) == -1 and rank_host(tot=-1) == -1
    host = G.cvxpnpl_ransac_guided_pool_host
    assert host(-1, 100, 8) == -1 and host(0, 3, 8) == -1 and host(0, 100, -1) == -1

    # a zero-size call is a no-op whatever the pointers
    assert rnk(F=0, off=z, q=z, order=z) == 0 and rnk(tot=0, off=z, q=z, order=z) == 0 and rnk(mx=0, off=z, q=z, order=z) == 0
    assert sample(F=0, tot=0, off=z, seeds=z, order=z, s2=z, s3=z, p2=z, p3=z) == 0 and sample(H=0, seeds=z, order=z, p2=z, p3=z) == 0
    for kw in (dict(F=0, tot=0), dict(A=0)):
        assert active(act=z, off=z, seeds=z, order=z, s2=z, s3=z, p2=z, p3=z, **kw) == 0
    assert active(Hr=0, act=z, seeds=z, order=z, p2=z, p3=z) == 0
    assert rank_host(F=0, off=z, q=z, order=z) == 0 and rank_host(tot=0, off=z, q=z, order=z) == 0


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

    assert os.path.exists(b.RANSAC_GUIDED_RESOURCES) and os.path.getmtime(b.RANSAC_GUIDED_RESOURCES) >= os.path.getmtime(b.RANSAC_GUIDED_OUT) - 1
    table = b.kernel_resources(b.RANSAC_GUIDED_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)
    assert golden["cvxng::rank_quality_kernel"]["lds"] == 256 * 8   # LDS is the ranking's tile of keys, and nothing else
    assert all(g["lds"] == 0 for k, g in golden.items() if "rank_quality" not in k)


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the other nine, no new name contains the short
    name of a kernel that was there before, and the third and the ninth library's tables still hold."""
    from cvxpnpl_amd import build as b

    b.build()
    others = {"solver": b.RESOURCES, "grad": b.GRAD_RESOURCES, "ransac": b.RANSAC_RESOURCES, "ransac_pnpl": b.RANSAC_PNPL_RESOURCES,
              "refine": b.REFINE_RESOURCES, "refine_grad": b.REFINE_GRAD_RESOURCES, "refine_robust": b.REFINE_ROBUST_RESOURCES,
              "refine_robust_grad": b.REFINE_ROBUST_GRAD_RESOURCES, "ransac_adaptive": b.RANSAC_ADAPTIVE_RESOURCES}
    tables = {lib: b.kernel_resources(path) for lib, path in others.items()}
    short = [k.split("::")[-1] for k in KERNELS]
    for lib, table in tables.items():
        assert table, lib
        assert not [k for k in table if "cvxng::" in k or any(n in k for n in short)], lib
        for k in table:
            assert not [n for n in short if k.split("::")[-1] in n], (lib, k)
    for lib, name in (("ransac", "ransac_kernel_resources.json"), ("ransac_adaptive", "ransac_adaptive_kernel_resources.json")):
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert set(tables[lib]) == set(golden), (lib, set(tables[lib]) ^ set(golden))
        problems = _compare(tables[lib], golden)
        assert not problems, "\n".join(problems)


PINNED = {0: 4, 1: 5, 2: 6, 10: 14, 15: 19, 16: 20, 50: 49, 100: 57, 256: 72, 512: 85, 1000: 100, 1023: 100, 1024: 100, 5000: 100}


def test_the_pool_on_the_host_equals_the_reference_exactly(G):
    from cvxpnpl_amd.ransac import pool_size

    host = G.cvxpnpl_ransac_guided_pool_host
    hs = np.concatenate([np.arange(1200), [2**31 - 2]]).astype(np.int64)
    for M in (4, 5, 64, 100, 700, 10**4):
        for pf in (0, 1, 7, 200, 1024, 10**6):
            ref = pools(hs, M, pf)
            got = np.array([host(int(h), M, pf) for h in hs], dtype=np.int64)
            assert np.array_equal(got, ref), (M, pf, hs[got != ref][:5], got[got != ref][:5], ref[got != ref][:5])
            assert (np.diff(got) >= 0).all(), (M, pf)                        # non-decreasing in h
            assert (got >= 4).all() and (got <= M).all(), (M, pf)
            below = hs < pf
            assert (got[below] <= 4 + hs[below]).all(), (M, pf)              # at most 4 + h before pool_full ...
            assert (got[~below] == M).all(), (M, pf)                         # ... the whole scene from pool_full on
            for h in (0, 1, 5, 63, 199, 200, 1023, 1199):                    # the vectorised reference against the linear one
                assert pool(h, M, pf) == ref[h], (M, pf, h)
    for h, n in PINNED.items():
        assert host(h, 100, 1024) == n and pool(h, 100, 1024) == n and pool_size(h, 100, 1024) == n, (h, n, host(h, 100, 1024))
    assert [host(h, 5, 8) for h in range(10)] == [4, 5, 5, 5, 5, 5, 5, 5, 5, 5]
    assert all(host(h, 4, pf) == 4 for h in (0, 1, 7, 1000) for pf in (0, 1, 8, 10**6))
    with pytest.raises(ValueError):
        pool_size(0, 100, -1)
    with pytest.raises(ValueError):
        pool_size(0, 3, 8)
    with pytest.raises(ValueError):
        pool_size(-1, 100, 8)


def _rank_host(G, sizes, quality):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    q = np.ascontiguousarray(quality, dtype=np.float64)
    order = np.full(off[-1] + 2, -9, dtype=np.int32)   # a guard word on either side
    assert G.cvxpnpl_ransac_guided_rank_host(len(sizes), off.ctypes.data, int(off[-1]), q.ctypes.data, order[1:].ctypes.data, 3) == 0
    assert order[0] == -9 and order[-1] == -9
    return off, order[1:-1]


def test_the_ranking_on_the_host_equals_the_reference(G):
    rs = np.random.RandomState(11)
    pats = [quality_patterns(m, rs) for m in SIZES]
    for name in pats[0]:
        off, order = _rank_host(G, SIZES, np.concatenate([p[name] for p in pats]))
        for f, m in enumerate(SIZES):
            mine, ref = order[off[f]:off[f + 1]], rank(pats[f][name])
            assert np.array_equal(mine, ref), (name, f, m)
            assert np.array_equal(np.sort(mine), np.arange(m)), (name, f)          # a permutation
            if name in ("all_equal", "ascending", "descending"):
                assert np.array_equal(mine, np.arange(m)[::-1] if name == "ascending" else np.arange(m)), (name, f)
    # NaN ranks with -inf, +0 ties with -0, +inf leads: by hand
    q = np.array([0.0, np.nan, -0.0, np.inf, -np.inf, 1.0, np.nan])
    _, order = _rank_host(G, [7], q)
    assert order.tolist() == [3, 5, 0, 2, 1, 4, 6] and rank(q).tolist() == order.tolist()


def test_the_reference_predicts_what_guidance_buys():
    """The CPU experiment behind the feature, on the restated sampler alone: M = 100, 70 % clutter, cap 1024.  The first all-inlier
    minimal set comes at hypothesis 0 in most scenes when guided by an informative quality, after about a hundred uniform draws, and
    later still under the reversed (adversarial) order."""
    from cvxpnpl_amd import synth

    rs = np.random.RandomState(3)
    first = {"uniform": [], "guided": [], "reversed": []}
    for f in range(40):
        inlier = np.zeros(100, dtype=bool)
        inlier[rs.choice(100, 30, replace=False)] = True
        q = planted_quality(inlier, rs)
        first["uniform"].append(first_all_inlier(synth.philox_minimal_sets(1024, 100, 4, 50 + f), inlier))
        first["guided"].append(first_all_inlier(guided_sets(1024, 100, rank(q), 1024, 50 + f), inlier))
        first["reversed"].append(first_all_inlier(guided_sets(1024, 100, rank(-q), 1024, 50 + f), inlier))
    med = {k: float(np.median([1024 if v < 0 else v for v in vs])) for k, vs in first.items()}
    print("median index of the first all-inlier minimal set:", med)
    assert med["guided"] == 0 and np.mean(np.array(first["guided"]) == 0) >= 0.9
    assert 40 <= med["uniform"] <= 250
    assert med["reversed"] > med["uniform"]
    # pool_full = 0 is the uniform sampler, and from pool_full on the sets are the uniform ones
    u = synth.philox_minimal_sets(300, 100, 4, 7)
    assert np.array_equal(guided_sets(300, 100, rank(rs.random_sample(100)), 0, 7), u)
    assert np.array_equal(guided_sets(300, 100, rank(rs.random_sample(100)), 200, 7)[200:], u[200:])
    order = rank(rs.random_sample(100))
    assert np.array_equal(guided_sets(64, 100, order, 200, 7, h0=192), guided_sets(256, 100, order, 200, 7)[192:])   # a round is a slice


def _scene(m, rs):
    return rs.random_sample((m, 2)), rs.random_sample((m, 3))


def test_guided_keywords_are_validated_on_the_host():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import inspect

    from cvxpnpl_amd.ransac import ransac_pnp_batch

    sig = inspect.signature(ransac_pnp_batch).parameters
    assert sig["quality"].default is None and sig["pool_full"].default is None
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3 = _scene(10, rs)
    b2, b3 = _scene(7, rs)
    qa, qb = rs.random_sample(10), rs.random_sample(7)
    lists = ([a2, b2], [a3, b3], K)
    packed = (np.concatenate([a2, b2]), np.concatenate([a3, b3]), K)
    with pytest.raises(ValueError, match="pool_full given without quality"):
        ransac_pnp_batch(*lists, pool_full=8)
    for bad in (-1, 1.5, "8", True, 2**31):
        with pytest.raises(ValueError, match="pool_full"):
            ransac_pnp_batch(*lists, quality=[qa, qb], pool_full=bad)
    with pytest.raises(ValueError, match="quality"):          # a scene's quality missing
        ransac_pnp_batch(*lists, quality=[qa])
    with pytest.raises(ValueError, match="quality"):          # a wrong length
        ransac_pnp_batch(*lists, quality=[qa, qb[:6]])
    with pytest.raises(ValueError, match="quality"):          # a wrong shape
        ransac_pnp_batch(*lists, quality=[qa, qb.reshape(7, 1)])
    with pytest.raises(ValueError, match="quality"):          # packed where a list is due
        ransac_pnp_batch(*lists, quality=np.concatenate([qa, qb]))
    with pytest.raises(ValueError, match="quality"):          # packed: the wrong total
        ransac_pnp_batch(*packed, sizes=[10, 7], quality=np.concatenate([qa, qb])[:16])
    with pytest.raises(ValueError, match="quality"):          # packed: two dimensions
        ransac_pnp_batch(*packed, sizes=[10, 7], quality=np.concatenate([qa, qb]).reshape(17, 1))
    with pytest.raises(ValueError, match="real"):             # not real numbers
        ransac_pnp_batch(*lists, quality=[qa.astype(np.complex128), qb])
    with pytest.raises(ValueError, match="n_hyp"):            # the earlier checks still come first
        ransac_pnp_batch(*lists, quality=[qa, qb], n_hyp=0)
    with pytest.raises(ValueError, match="needs 4"):
        ransac_pnp_batch([a2, b2[:3]], [a3, b3[:3]], K, quality=[qa, qb[:3]])
    with pytest.raises(ValueError, match="confidence"):
        ransac_pnp_batch(*lists, quality=[qa, qb], confidence=1.0)
