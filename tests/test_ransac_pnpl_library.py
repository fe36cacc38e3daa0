"""The library of RANSAC over points and lines (libcvxpnpl_amd_ransac_pnpl.so, include/cvxpnpl_amd_ransac_pnpl.h): it builds by
cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels
free of scratch and spills (tests/golden/ransac_pnpl_kernel_resources.json) and leaves the other three libraries alone; and the
host-side validation of ransac_pnpl_batch.  No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_pnpl_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxnl::sample_assemble_kernel", "cvxnl::score_kernel", "cvxnl::select_kernel", "cvxnl::assemble_consensus_kernel",
           "cvxnl::refit_update_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_pnpl()
    assert os.path.exists(build.RANSAC_PNPL_OUT)
    return _lib.ransac_pnpl_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_pnpl.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_PNPL_EXPORTS), declared ^ set(_lib.RANSAC_PNPL_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_PNPL_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library():
    from cvxpnpl_amd import build as b

    assert b.ransac_pnpl_compile_cmd("x")[:-1] == b.ransac_compile_cmd("x")[:-1]


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_pnpl_last_error
    nan = float("nan")

    def sample(F=2, H=8, op=p, n_p=10, ol=p, n_l=6, seeds=p, p2=p, p3=p, l2=p, l3=p, K=p, per=0, idx=None, Q=p, B=p):
        return G.cvxpnpl_ransac_pnpl_sample_assemble(F, H, op, n_p, ol, n_l, seeds, p2, p3, l2, l3, K, per, idx, Q, B, None)

    assert sample(op=None) == -1
    assert b"cvxpnpl_ransac_pnpl_sample_assemble: bad arguments" in err() and b"offsets" in err()
    assert sample(ol=None) == -1 and sample(F=-1) == -1 and sample(H=-8) == -1 and sample(n_p=-1) == -1 and sample(n_l=-1) == -1
    assert sample(seeds=None) == -1 and sample(K=None) == -1 and sample(Q=None) == -1 and sample(B=None) == -1 and sample(per=2) == -1
    assert sample(p2=None) == -1 and b"point pointer" in err()
    assert sample(l3=None) == -1 and b"line pointer" in err()

    def score(F=2, H=8, op=p, n_p=10, ol=p, n_l=6, R=p, t=p, st=None, um=5, K=p, per=0, p2=p, p3=p, l2=p, l3=p, th=2.0, cnt=p):
        return G.cvxpnpl_ransac_pnpl_score(F, H, op, n_p, ol, n_l, R, t, st, um, K, per, p2, p3, l2, l3, th, cnt, None)

    assert score(R=None) == -1
    assert b"cvxpnpl_ransac_pnpl_score: bad arguments" in err()
    assert score(per=2) == -1 and score(th=nan) == -1 and score(th=-1.0) == -1 and score(n_l=-1) == -1 and score(cnt=None) == -1
    assert score(ol=None) == -1 and score(l2=None) == -1 and score(p3=None) == -1 and score(H=-1) == -1

    def select(F=2, H=8, op=p, n_p=10, ol=p, n_l=6, cnt=p, R=p, t=p, st=p, K=p, per=0, p2=p, p3=p, l2=p, l3=p, th=2.0, oR=p, ot=p, head=p, mp=p, ml=p):
        return G.cvxpnpl_ransac_pnpl_select(F, H, op, n_p, ol, n_l, cnt, R, t, st, K, per, p2, p3, l2, l3, th, oR, ot, head, mp, ml, None)

    assert select(H=0) == -1                                   # no hypotheses
    assert b"cvxpnpl_ransac_pnpl_select: bad arguments" in err()
    assert select(st=None) == -1 and select(mp=None) == -1 and select(ml=None) == -1 and select(th=-1.0) == -1 and select(th=nan) == -1
    assert select(head=None) == -1 and select(per=-1) == -1 and select(F=-2) == -1

    def consensus(F=2, op=p, n_p=10, ol=p, n_l=6, p2=p, p3=p, l2=p, l3=p, mp=p, ml=p, K=p, per=0, B=p, Q=p, cnt=p):
        return G.cvxpnpl_ransac_pnpl_assemble_consensus(F, op, n_p, ol, n_l, p2, p3, l2, l3, mp, ml, K, per, B, Q, cnt, None)

    assert consensus(mp=None) == -1
    assert b"cvxpnpl_ransac_pnpl_assemble_consensus: bad arguments" in err()
    assert consensus(ml=None) == -1 and consensus(Q=None) == -1 and consensus(op=None) == -1 and consensus(per=3) == -1 and consensus(n_p=-4) == -1

    def refit(F=2, op=p, n_p=10, ol=p, n_l=6, fR=p, ft=p, fs=p, fc=p, K=p, per=0, p2=p, p3=p, l2=p, l3=p, th=2.0, R=p, t=p, head=p, mp=p, ml=p):
        return G.cvxpnpl_ransac_pnpl_refit_update(F, op, n_p, ol, n_l, fR, ft, fs, fc, K, per, p2, p3, l2, l3, th, R, t, head, mp, ml, None)

    assert refit(fs=None) == -1
    assert b"cvxpnpl_ransac_pnpl_refit_update: bad arguments" in err()
    assert refit(per=7) == -1 and refit(head=None) == -1 and refit(ml=None) == -1 and refit(th=nan) == -1 and refit(F=-1) == -1

    # a zero-size call is a no-op whatever the pointers
    z = None
    assert sample(F=0, op=z, ol=z, seeds=z, p2=z, p3=z, l2=z, l3=z, K=z, Q=z, B=z, n_p=0, n_l=0) == 0
    assert sample(H=0, seeds=z, K=z, Q=z, B=z) == 0
    assert score(F=0, op=z, ol=z, R=z, t=z, K=z, p2=z, p3=z, l2=z, l3=z, cnt=z, n_p=0, n_l=0) == 0
    assert score(H=0, R=z, t=z, K=z, cnt=z) == 0
    assert select(F=0, op=z, ol=z, cnt=z, R=z, t=z, st=z, K=z, p2=z, p3=z, l2=z, l3=z, oR=z, ot=z, head=z, mp=z, ml=z, n_p=0, n_l=0) == 0
    assert consensus(F=0, op=z, ol=z, p2=z, p3=z, l2=z, l3=z, mp=z, ml=z, K=z, B=z, Q=z, cnt=z, n_p=0, n_l=0) == 0
    assert refit(F=0, op=z, ol=z, fR=z, ft=z, fs=z, fc=z, K=z, p2=z, p3=z, l2=z, l3=z, R=z, t=z, head=z, mp=z, ml=z, n_p=0, n_l=0) == 0


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

    assert os.path.exists(b.RANSAC_PNPL_RESOURCES) and os.path.getmtime(b.RANSAC_PNPL_RESOURCES) >= os.path.getmtime(b.RANSAC_PNPL_OUT) - 1
    table = b.kernel_resources(b.RANSAC_PNPL_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the solver, grad or ransac libraries, and each of
    those still matches its own committed table (for the ransac library: after the move of the shared functions into ransac_common.h)."""
    import test_kernel_resources as tkr
    from cvxpnpl_amd import build as b

    b.build()
    tables = {"solver": b.kernel_resources(), "grad": b.kernel_resources(b.GRAD_RESOURCES), "ransac": b.kernel_resources(b.RANSAC_RESOURCES)}
    for lib, table in tables.items():
        assert table, lib
        assert not [k for k in table if "cvxnl::" in k or "sample_assemble_kernel" in k], lib
    problems = tkr._compare(tables["solver"], json.load(open(tkr.GOLDEN)))
    assert not problems, "\n".join(problems)
    for lib, name in (("grad", "grad_kernel_resources.json"), ("ransac", "ransac_kernel_resources.json")):
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert set(tables[lib]) == set(golden), (lib, set(tables[lib]) ^ set(golden))
        problems = _compare(tables[lib], golden)
        assert not problems, "\n".join(problems)


def _scene(p, l, rs):
    return rs.random_sample((p, 2)), rs.random_sample((p, 3)), rs.random_sample((l, 2, 2)), rs.random_sample((l, 2, 3))


def test_scene_sets_are_validated_on_the_host():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    assert ca.ransac_pnpl_batch is rn.ransac_pnpl_batch and ca.ransac_pnl_batch is rn.ransac_pnl_batch
    assert ca.ransac_pnpl is rn.ransac_pnpl and ca.ransac_pnl is rn.ransac_pnl
    run = rn.ransac_pnpl_batch
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3, al2, al3 = _scene(10, 5, rs)
    b2, b3, bl2, bl3 = _scene(2, 3, rs)
    with pytest.raises(ValueError, match="no scenes"):                          # an empty scene set
        run([], [], [], [], K)
    with pytest.raises(ValueError, match="no scenes"):
        run(None, None, None, None, K)
    with pytest.raises(ValueError, match="no scenes"):
        run(np.zeros((0, 2)), np.zeros((0, 2, 2)), np.zeros((0, 3)), np.zeros((0, 2, 3)), K, sizes=[], line_sizes=[])
    with pytest.raises(ValueError, match="needs 4"):                            # fewer than four correspondences in total
        run([a2, b2], [al2, bl2[:1]], [a3, b3], [al3, bl3[:1]], K)
    with pytest.raises(ValueError, match="needs 4"):
        run([a2, b2], None, [a3, b3], None, K)
    with pytest.raises(ValueError, match="needs 4"):
        rn.ransac_pnl_batch([al2, bl2], [al3, bl3], K)
    with pytest.raises(ValueError, match="needs 4"):
        rn.ransac_pnpl(b2, bl2[:1], b3, bl3[:1], K)
    with pytest.raises(ValueError, match="needs 4"):
        rn.ransac_pnl(bl2, bl3, K)
    with pytest.raises(ValueError, match="needs 4"):
        run(np.concatenate([a2, b2]), np.concatenate([al2, bl2]), np.concatenate([a3, b3]), np.concatenate([al3, bl3]), K, sizes=[11, 1], line_sizes=[6, 2])
    with pytest.raises(ValueError, match="2D points for"):                      # 2D and 3D lengths that differ: points
        run([a2, b2], [al2, bl2], [a3, b3[:1]], [al3, bl3], K)
    with pytest.raises(ValueError, match="2D lines for"):                       # ... lines
        run([a2, b2], [al2, bl2], [a3, b3], [al3, bl3[:2]], K)
    with pytest.raises(ValueError, match="2D points for"):
        run(np.concatenate([a2, b2]), None, np.concatenate([a3, b3])[:-1], None, K, sizes=[10, 2])
    with pytest.raises(ValueError, match="2D lines for"):
        run(None, np.concatenate([al2, bl2]), None, np.concatenate([al3, bl3])[:-1], K, line_sizes=[5, 3])
    with pytest.raises(ValueError, match="scenes of 2D points"):
        run([a2, b2], [al2, bl2], [a3], [al3, bl3], K)
    with pytest.raises(ValueError, match="scenes of points for"):               # different numbers of point scenes and line scenes
        run([a2, b2], [al2], [a3, b3], [al3], K)
    with pytest.raises(ValueError, match="scenes of points for"):
        run(np.concatenate([a2, b2]), [al2], np.concatenate([a3, b3]), [al3], K, sizes=[10, 2])
    with pytest.raises(ValueError, match="add up"):                             # sizes that do not add up
        run(np.concatenate([a2, b2]), [al2, bl2], np.concatenate([a3, b3]), [al3, bl3], K, sizes=[10, 3])
    with pytest.raises(ValueError, match="add up"):
        run([a2, b2], np.concatenate([al2, bl2]), [a3, b3], np.concatenate([al3, bl3]), K, line_sizes=[5, 2])
    with pytest.raises(ValueError, match="go together"):
        run([a2, b2], [al2, bl2], None, [al3, bl3], K)
    for bad_K in (np.eye(4), np.zeros((3, 3, 3)), np.zeros((1, 3, 3)), np.zeros(9)):   # K not [3,3] or [F,3,3]
        with pytest.raises(ValueError, match="K must be"):
            run([a2, b2], [al2, bl2], [a3, b3], [al3, bl3], bad_K)
    with pytest.raises(ValueError, match="seeds"):                              # a wrong number of seeds
        run([a2, b2], [al2, bl2], [a3, b3], [al3, bl3], K, seed=[1, 2, 3])
    with pytest.raises(ValueError, match="expected 2D points"):
        run([a3, b2], [al2, bl2], [a3, b3], [al3, bl3], K)
    with pytest.raises(ValueError, match="expected 3D lines"):
        run([a2, b2], [al2, bl2], [a3, b3], [al2, bl3], K)
    with pytest.raises(ValueError):                                              # packed arrays without sizes
        run(np.concatenate([a2, b2]), None, np.concatenate([a3, b3]), None, K)
    # what IS a valid set passes the validation: single scenes without points or without lines, None entries, empty arrays
    ps, ls = rn._check_pnpl_scenes([a2, None, np.zeros((0, 2))], [None, al2, al2[:4]], [a3, None, np.zeros((0, 3))],
                                   [np.zeros((0, 2, 3)), al3, al3[:4]], K, None, None)
    assert ps == [10, 0, 0] and ls == [0, 5, 4]
    ps, ls = rn._check_pnpl_scenes(None, np.concatenate([al2, al2]), None, np.concatenate([al3, al3]), np.zeros((2, 3, 3)), None, [4, 6])
    assert ps == [0, 0] and ls == [4, 6]


def test_synthetic_scene_of_points_and_lines():
    from cvxpnpl_amd import synth

    d = synth.make_ransac_pnpl(40, 30, outlier_frac=0.25, sigma=0.0, seed=5)
    assert d["pts_2d"].shape == (40, 2) and d["pts_3d"].shape == (40, 3) and d["line_2d"].shape == (30, 2, 2) and d["line_3d"].shape == (30, 2, 3)
    assert int((~d["inlier_pts"]).sum()) == 10 and int((~d["inlier_lines"]).sum()) == 8
    R, t, K = d["R_gt"], d["t_gt"], d["K"]
    err = np.linalg.norm(synth.project(d["pts_3d"][None], K, R[None], t[None])[0] - d["pts_2d"], axis=1)
    assert err[d["inlier_pts"]].max() < 1e-9 and err[~d["inlier_pts"]].min() > 1e-3
    e2 = synth.project(d["line_3d"].reshape(1, -1, 3), K, R[None], t[None])[0].reshape(30, 2, 2)
    lerr = np.abs(e2 - d["line_2d"]).max(axis=(1, 2))
    assert lerr[d["inlier_lines"]].max() < 1e-9 and lerr[~d["inlier_lines"]].min() > 1e-3
    only = synth.make_ransac_pnpl(0, 12, outlier_frac=0.5, seed=1)
    assert only["pts_2d"].shape == (0, 2) and int(only["inlier_lines"].sum()) == 6
