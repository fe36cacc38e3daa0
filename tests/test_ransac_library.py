"""The multi-scene RANSAC library (libcvxpnpl_amd_ransac.so, include/cvxpnpl_amd_ransac.h): it builds by cross-compilation, exports what
its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels free of scratch and spills
(tests/golden/ransac_kernel_resources.json), and leaves the solver library alone; and the host-side validation of ransac_pnp_batch.
No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("sample_scenes_kernel", "score_scenes_kernel", "select_scenes_kernel", "assemble_consensus_kernel", "refit_update_scenes_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac()
    assert os.path.exists(build.RANSAC_OUT)
    return _lib.ransac_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_EXPORTS), declared ^ set(_lib.RANSAC_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    # the dynamic symbol table: every cvxpnpl_* function the library defines is one the header declares
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_last_error

    assert G.cvxpnpl_ransac_sample_scenes(2, 8, None, 10, p, p, p, None, None, p, p, None, None) == -1
    assert b"cvxpnpl_ransac_sample_scenes: bad arguments" in err() and b"d_offsets" in err()
    assert G.cvxpnpl_ransac_sample_scenes(-1, 8, p, 10, p, p, p, None, None, p, p, None, None) == -1
    assert G.cvxpnpl_ransac_sample_scenes(2, -8, p, 10, p, p, p, None, None, p, p, None, None) == -1
    assert G.cvxpnpl_ransac_sample_scenes(2, 8, p, 10, None, p, p, None, None, p, p, None, None) == -1       # no seeds
    assert G.cvxpnpl_ransac_sample_scenes(2, 8, p, 10, p, p, p, p, None, p, p, None, None) == -1             # K without K_hyp
    assert G.cvxpnpl_ransac_sample_scenes(2, 8, p, 10, p, None, p, None, None, p, p, None, None) == -1       # no scene

    assert G.cvxpnpl_ransac_score_scenes(2, 8, p, 10, None, p, None, 5, p, 0, p, p, 2.0, p, None) == -1
    assert b"cvxpnpl_ransac_score_scenes: bad arguments" in err()
    assert G.cvxpnpl_ransac_score_scenes(2, 8, p, 10, p, p, None, 5, p, 2, p, p, 2.0, p, None) == -1         # K_per_scene
    assert G.cvxpnpl_ransac_score_scenes(2, 8, p, 10, p, p, None, 5, p, 0, p, p, float("nan"), p, None) == -1
    assert G.cvxpnpl_ransac_score_scenes(2, 8, p, -1, p, p, None, 5, p, 0, p, p, 2.0, p, None) == -1

    assert G.cvxpnpl_ransac_select_scenes(2, 0, p, 10, p, p, p, p, p, 0, p, p, 2.0, p, p, p, p, None) == -1    # no hypotheses
    assert b"cvxpnpl_ransac_select_scenes: bad arguments" in err()
    assert G.cvxpnpl_ransac_select_scenes(2, 8, p, 10, p, p, p, None, p, 0, p, p, 2.0, p, p, p, p, None) == -1  # no status
    assert G.cvxpnpl_ransac_select_scenes(2, 8, p, 10, p, p, p, p, p, 0, p, p, 2.0, p, p, p, None, None) == -1  # no mask
    assert G.cvxpnpl_ransac_select_scenes(2, 8, p, 10, p, p, p, p, p, 0, p, p, -1.0, p, p, p, p, None) == -1

    assert G.cvxpnpl_ransac_assemble_consensus(2, p, 10, p, p, None, p, 0, p, p, p, None) == -1
    assert b"cvxpnpl_ransac_assemble_consensus: bad arguments" in err()
    assert G.cvxpnpl_ransac_assemble_consensus(2, p, 10, p, p, p, p, 0, p, None, p, None) == -1
    assert G.cvxpnpl_ransac_assemble_consensus(2, None, 10, p, p, p, p, 0, p, p, p, None) == -1

    assert G.cvxpnpl_ransac_refit_update_scenes(2, p, 10, p, p, None, p, p, 0, p, p, 2.0, p, p, p, p, None) == -1
    assert b"cvxpnpl_ransac_refit_update_scenes: bad arguments" in err()
    assert G.cvxpnpl_ransac_refit_update_scenes(2, p, 10, p, p, p, p, p, 7, p, p, 2.0, p, p, p, p, None) == -1
    assert G.cvxpnpl_ransac_refit_update_scenes(2, p, 10, p, p, p, p, p, 0, p, p, 2.0, p, p, None, p, None) == -1

    # a zero-size call is a no-op whatever the pointers
    assert G.cvxpnpl_ransac_sample_scenes(0, 8, None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert G.cvxpnpl_ransac_sample_scenes(2, 0, p, 10, None, p, p, None, None, None, None, None, None) == 0
    assert G.cvxpnpl_ransac_score_scenes(0, 8, None, 0, None, None, None, 5, None, 0, None, None, 2.0, None, None) == 0
    assert G.cvxpnpl_ransac_score_scenes(2, 0, p, 10, None, None, None, 5, None, 0, p, p, 2.0, None, None) == 0
    assert G.cvxpnpl_ransac_select_scenes(0, 8, None, 0, None, None, None, None, None, 0, None, None, 2.0, None, None, None, None, None) == 0
    assert G.cvxpnpl_ransac_assemble_consensus(0, None, 0, None, None, None, None, 0, None, None, None, None) == 0
    assert G.cvxpnpl_ransac_refit_update_scenes(0, None, 0, None, None, None, None, None, 0, None, None, 2.0, None, None, None, None, None) == 0


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.RANSAC_RESOURCES) and os.path.getmtime(b.RANSAC_RESOURCES) >= os.path.getmtime(b.RANSAC_OUT) - 1
    table = b.kernel_resources(b.RANSAC_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden), set(table) ^ set(golden)
    assert sorted(k.split("::")[-1] for k in table) == sorted(KERNELS)
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
    assert not problems, "\n".join(problems)


def test_the_solver_library_is_left_alone():
    """The new kernels live in their own library: none of them appears in the solver's remarks, and the solver's own table still holds."""
    import test_kernel_resources as tkr
    from cvxpnpl_amd import build as b

    b.build()
    table = b.kernel_resources()
    assert not [k for k in table if any(n in k for n in KERNELS) or "cvxn::" in k]
    problems = tkr._compare(table, json.load(open(tkr.GOLDEN)))
    assert not problems, "\n".join(problems)


def _scene(m, rs):
    return rs.random_sample((m, 2)), rs.random_sample((m, 3))


def test_scene_sets_are_validated_on_the_host():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import cvxpnpl_amd as ca
    from cvxpnpl_amd.ransac import ransac_pnp_batch

    assert ca.ransac_pnp_batch is ransac_pnp_batch
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3 = _scene(10, rs)
    b2, b3 = _scene(7, rs)
    with pytest.raises(ValueError, match="fewer|needs 4|minimal"):      # a scene with fewer than 4 correspondences
        ransac_pnp_batch([a2, b2[:3]], [a3, b3[:3]], K)
    with pytest.raises(ValueError, match="2D points for"):              # mismatched 2D and 3D lengths
        ransac_pnp_batch([a2, b2], [a3, b3[:6]], K)
    with pytest.raises(ValueError, match="scenes of 2D"):
        ransac_pnp_batch([a2, b2], [a3], K)
    with pytest.raises(ValueError, match="add up"):                     # sum(sizes) != sum M
        ransac_pnp_batch(np.concatenate([a2, b2]), np.concatenate([a3, b3]), K, sizes=[10, 6])
    with pytest.raises(ValueError, match="2D points for"):
        ransac_pnp_batch(np.concatenate([a2, b2]), np.concatenate([a3, b3])[:-1], K, sizes=[10, 7])
    with pytest.raises(ValueError, match="needs 4"):
        ransac_pnp_batch(np.concatenate([a2, b2]), np.concatenate([a3, b3]), K, sizes=[14, 3])
    with pytest.raises(ValueError, match="no scenes"):                  # F == 0
        ransac_pnp_batch([], [], K)
    with pytest.raises(ValueError, match="no scenes"):
        ransac_pnp_batch(np.zeros((0, 2)), np.zeros((0, 3)), K, sizes=[])
    for bad_K in (np.eye(4), np.zeros((3, 3, 3)), np.zeros((1, 3, 3)), np.zeros(9)):   # K not [3,3] or [F,3,3]
        with pytest.raises(ValueError, match="K must be"):
            ransac_pnp_batch([a2, b2], [a3, b3], bad_K)
    with pytest.raises(ValueError, match="seeds"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, seed=[1, 2, 3])
    with pytest.raises(ValueError, match="expected pts_2d"):
        ransac_pnp_batch([a3, b2], [a3, b3], K)
    with pytest.raises(ValueError):                                      # packed arrays without sizes
        ransac_pnp_batch(np.concatenate([a2, b2]), np.concatenate([a3, b3]), K)
