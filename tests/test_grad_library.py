"""The backward-pass library (libcvxpnpl_amd_grad.so, include/cvxpnpl_amd_grad.h): exports, argument checks and the kernel resources
of its build against tests/golden/grad_kernel_resources.json -- no GPU needed (hipcc cross-compiles)."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "grad_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move; occupancy, LDS, scratch and spills are exact


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_grad()
    return _lib.grad_lib()


def test_header_symbols_are_exported(G):
    from cvxpnpl_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_grad.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.GRAD_EXPORTS), declared ^ set(_lib.GRAD_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None


def test_bad_arguments_are_rejected_without_gpu(G):
    args = [4, 0, None, None, 0, None, None, None, 0, None, None, None, 1, None, None, None, None, None, None, None, None]
    assert G.cvxpnpl_pose_vjp_batch(*args, None) == -1
    assert b"cvxpnpl_pose_vjp_batch: bad arguments" in G.cvxpnpl_grad_last_error()
    assert G.cvxpnpl_pose_vjp_host(*args, 1) == -1
    # an empty batch is a no-op whatever the pointers
    assert G.cvxpnpl_pose_vjp_batch(0, 10, C.c_void_p(8), C.c_void_p(8), 0, None, None, C.c_void_p(8), 0, None, None, None, 1, *([None] * 8), None) == 0


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.GRAD_RESOURCES) and os.path.getmtime(b.GRAD_RESOURCES) >= os.path.getmtime(b.GRAD_OUT) - 1
    table = b.kernel_resources(b.GRAD_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden), set(table) ^ set(golden)
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
