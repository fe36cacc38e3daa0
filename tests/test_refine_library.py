"""The library of the reprojection refinement (libcvxpnpl_amd_refine.so, include/cvxpnpl_amd_refine.h): it builds by cross-compilation,
exports what its header declares and nothing else, rejects bad arguments before it touches a device, guards the size of its options,
keeps its kernels free of scratch and spills (tests/golden/refine_kernel_resources.json) and leaves the other four libraries' compile
commands alone; and the host-side validation of the Python entry points.  No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refine_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_ransac_pnpl_library.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxr::refine_group_kernel<1>", "cvxr::refine_group_kernel<2>", "cvxr::refine_group_kernel<4>", "cvxr::refine_group_kernel<0>",
           "cvxr::refine_scenes_kernel", "cvxr::cov_group_kernel", "cvxr::cov_scenes_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_refine()
    assert os.path.exists(build.REFINE_OUT)
    return _lib.refine_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_refine.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.REFINE_EXPORTS), declared ^ set(_lib.REFINE_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.REFINE_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared
    assert not [ln for ln in nm.splitlines() if re.search(r"err_buf|bad_args|launched|check_\w+|host_problem|host_weights|host_grads|fill_batch|fill_scenes|for_chunks", ln)], "the shared argument checks are exported"
    assert G.cvxpnpl_refine_version().startswith(b"cvxpnpl_amd_refine")


def test_the_other_compile_commands_are_unchanged():
    from cvxpnpl_amd import build as b

    flags = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value"]
    assert b.compile_cmd("x")[1:] == flags + ["-mllvm", "-enable-ipra=0", "-o", "x", b.SRC, b.LANE_SRC, b.HOST_SRC]
    assert b.grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.GRAD_SRC, b.GRAD_HOST_SRC]
    assert b.ransac_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_SRC]
    assert b.ransac_pnpl_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_PNPL_SRC]
    assert b.refine_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_SRC, b.REFINE_HOST_SRC]     # the grad library's flags


def _calls(G):
    from cvxpnpl_amd._lib import RefineOpts

    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it reads or launches anything

    def opts(size=None, max_iters=30, step_tol=1e-10, lambda0=1e-3, sigma_px=0.0):
        return RefineOpts(C.sizeof(RefineOpts) if size is None else size, max_iters, step_tol, lambda0, sigma_px)

    def batch(fn, B=2, n_p=10, p2=p, p3=p, n_l=6, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=5, mp=None, ml=None, o=None,
              oR=p, ot=p, cost=p, it=p, ost=p, nl=p, cov=None, last=None):
        return fn(B, n_p, p2, p3, n_l, l2, l3, K, per, R, t, st, stride, admit, mp, ml, None if o is None else C.byref(o), oR, ot, cost, it, ost, nl, cov,
                  last)

    def scenes(F=2, op=p, n_pts=10, ol=p, n_lines=6, p2=p, p3=p, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=5, mp=None, ml=None,
               o=None, oR=p, ot=p, cost=p, it=p, ost=p, nl=p, cov=None):
        return G.cvxpnpl_refine_scenes(F, op, n_pts, ol, n_lines, p2, p3, l2, l3, K, per, R, t, st, stride, admit, mp, ml,
                                       None if o is None else C.byref(o), oR, ot, cost, it, ost, nl, cov, None)

    return p, opts, batch, scenes


def test_bad_arguments_are_rejected_without_gpu(G):
    p, opts, batch, scenes = _calls(G)
    err = G.cvxpnpl_refine_last_error
    nan, inf = float("nan"), float("inf")
    for fn, name, last in ((G.cvxpnpl_refine_batch, b"cvxpnpl_refine_batch:", None), (G.cvxpnpl_refine_batch_host, b"cvxpnpl_refine_batch_host:", 1)):
        def run(**kw):
            return batch(fn, last=last, **kw)

        assert run(B=-1) == -1 and err().startswith(name) and b"bad arguments" in err()
        assert run(n_p=-1) == -1 and run(n_l=-2) == -1
        assert run(p2=None) == -1 and b"correspondence pointer" in err()
        assert run(l3=None) == -1 and run(p3=None) == -1 and run(l2=None) == -1
        assert run(K=None) == -1 and run(R=None) == -1 and run(t=None) == -1
        assert run(per=2) == -1 and run(per=-1) == -1 and b"0 or 1" in err()
        assert run(oR=None) == -1 and run(ot=None) == -1 and run(cost=None) == -1 and run(it=None) == -1 and run(ost=None) == -1 and run(nl=None) == -1
        assert run(st=p, stride=-1) == -1 and b"status_stride" in err()
        assert run(o=opts(max_iters=-1)) == -1 and b"max_iters" in err()
        assert run(o=opts(step_tol=-1.0)) == -1 and run(o=opts(step_tol=nan)) == -1 and run(o=opts(step_tol=inf)) == -1 and b"step_tol" in err()
        assert run(o=opts(lambda0=nan)) == -1 and run(o=opts(lambda0=-1e-3)) == -1
        assert run(o=opts(sigma_px=-1.0)) == -1 and run(o=opts(sigma_px=nan)) == -1 and b"sigma_px" in err()
        assert run(o=opts(size=8)) == -1 and b"struct_size" in err()                       # the size guard
        assert run(o=opts(size=C.sizeof(type(opts())) + 8)) == -1
        z = None                                                                            # a zero-size call is a no-op whatever the pointers
        assert run(B=0, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, oR=z, ot=z, cost=z, it=z, ost=z, nl=z, per=7, o=opts(size=3)) == 0
    assert scenes(F=-1) == -1 and err().startswith(b"cvxpnpl_refine_scenes:")
    assert scenes(n_pts=-1) == -1 and scenes(n_lines=-1) == -1
    assert scenes(op=None) == -1 and scenes(ol=None) == -1 and b"offsets" in err()
    assert scenes(p3=None) == -1 and scenes(l2=None) == -1 and scenes(K=None) == -1 and scenes(R=None) == -1 and scenes(per=3) == -1
    assert scenes(ost=None) == -1 and scenes(o=opts(max_iters=-5)) == -1 and scenes(o=opts(size=0)) == -1 and scenes(o=opts(step_tol=nan)) == -1
    z = None
    assert scenes(F=0, op=z, ol=z, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, oR=z, ot=z, cost=z, it=z, ost=z, nl=z, n_pts=0, n_lines=0) == 0


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

    assert os.path.exists(b.REFINE_RESOURCES) and os.path.getmtime(b.REFINE_RESOURCES) >= os.path.getmtime(b.REFINE_OUT) - 1
    table = b.kernel_resources(b.REFINE_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)


def test_python_entry_points_validate_before_they_ask_for_a_gpu():
    """Every ValueError below is raised before _require_gpu: this test runs on a machine without a GPU."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import refine as rf

    assert ca.refine_pose_batch is rf.refine_pose_batch and ca.refine_scenes is rf.refine_scenes and ca.refine_pose_batch_host is rf.refine_pose_batch_host
    B = 3
    R, t = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1), torch.zeros(B, 3, dtype=torch.float64)
    p2, p3, K = torch.zeros(B, 5, 2, dtype=torch.float64), torch.zeros(B, 5, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU path"):                                  # device
        rf.refine_pose_batch(R, t, pts_2d=p2, pts_3d=p3, K=K)
    with pytest.raises(ValueError, match="torch tensor"):
        rf.refine_pose_batch(R.numpy(), t, pts_2d=p2, pts_3d=p3, K=K)
    with pytest.raises(ValueError, match="max_iters"):
        rf.refine_pose_batch(R, t, pts_2d=p2, pts_3d=p3, K=K, max_iters=-1)
    with pytest.raises(ValueError, match="step_tol"):
        rf.refine_pose_batch(R, t, pts_2d=p2, pts_3d=p3, K=K, step_tol=float("nan"))
    meta = torch.device("meta")                                                           # a stand-in for a second device: nothing is computed on it
    Rm, tm, p2m, p3m, Km = R, t, p2, p3, K
    for bad, match in ((dict(t=tm.float()), "dtype"), (dict(t=tm[:, :2]), "shape"), (dict(t=t.to(meta)), "on meta"), (dict(pts_2d=p2m[:, :4]), "shape"),
                       (dict(pts_2d=p2m.float()), "dtype"), (dict(pts_2d=None), "go together"), (dict(K=Km[:2]), "K must be"),
                       (dict(K=Km.float()), "dtype"), (dict(status=torch.zeros(B, dtype=torch.int64, device="cpu")), "status"),
                       (dict(mask_pts=torch.ones(B, 5, dtype=torch.bool, device="cpu")), "dtype"),
                       (dict(mask_pts=torch.ones(B, 4, dtype=torch.uint8, device="cpu")), "shape"),
                       (dict(pts_3d=p3m.transpose(0, 1).contiguous().transpose(0, 1)), "contiguous"), (dict(pts_2d=None, pts_3d=None), "at least one")):
        kw = dict(R=Rm, t=tm, pts_2d=p2m, pts_3d=p3m, K=Km)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            rf.refine_pose_batch(**kw)
    with pytest.raises(ValueError, match="ransac.Scenes"):
        rf.refine_scenes(object(), R, t)
    with pytest.raises(ValueError):                                                      # the host form checks shapes too
        rf.refine_pose_batch_host(np.eye(3)[None], np.zeros((2, 3)), pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(3))
    with pytest.raises(ValueError, match="K must be"):
        rf.refine_pose_batch_host(np.eye(3)[None], np.zeros((1, 3)), pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(4))
