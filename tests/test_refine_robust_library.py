"""The library of the robust refinement (libcvxpnpl_amd_refine_robust.so, include/cvxpnpl_amd_refine_robust.h): it builds by
cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels
free of scratch and spills (tests/golden/refine_robust_kernel_resources.json) and leaves the other six libraries' compile commands alone;
the host-side validation of the Python entry points; and the host path compiled from source under ASan + UBSan in a stand-alone program
(tests/hostsim/refine_robust_sanitize_main.cpp).  No GPU needed."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refine_robust_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_refine_library.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxrb::refine_robust_group_kernel<1>", "cvxrb::refine_robust_group_kernel<2>", "cvxrb::refine_robust_group_kernel<4>",
           "cvxrb::refine_robust_group_kernel<0>", "cvxrb::refine_robust_scenes_kernel", "cvxrb::robust_w_group_kernel", "cvxrb::robust_w_scenes_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_refine_robust()
    assert os.path.exists(build.REFINE_ROBUST_OUT)
    return _lib.refine_robust_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_refine_robust.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.REFINE_ROBUST_EXPORTS), declared ^ set(_lib.REFINE_ROBUST_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.REFINE_ROBUST_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared
    assert not [ln for ln in nm.splitlines() if re.search(r"err_buf|bad_args|launched|check_\w+|host_problem|host_weights|host_grads|fill_batch|fill_scenes|for_chunks", ln)], "the shared argument checks are exported"
    assert G.cvxpnpl_refine_robust_version().startswith(b"cvxpnpl_amd_refine_robust")
    assert C.sizeof(_lib.RefineRobustOpts) == 40                                           # {u32, i32, f64, f64, i32, pad, f64}


def test_the_other_compile_commands_are_unchanged_and_the_new_one_has_the_grad_flags():
    from cvxpnpl_amd import build as b

    flags = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value"]
    assert b.compile_cmd("x")[1:] == flags + ["-mllvm", "-enable-ipra=0", "-o", "x", b.SRC, b.LANE_SRC, b.HOST_SRC]
    assert b.grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.GRAD_SRC, b.GRAD_HOST_SRC]
    assert b.ransac_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_SRC]
    assert b.ransac_pnpl_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_PNPL_SRC]
    assert b.refine_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_SRC, b.REFINE_HOST_SRC]
    assert b.refine_grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_GRAD_SRC, b.REFINE_GRAD_HOST_SRC]
    assert b.refine_robust_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_ROBUST_SRC, b.REFINE_ROBUST_HOST_SRC]
    assert b.refine_robust_compile_cmd("x")[:-2] == b.grad_compile_cmd("x")[:-2] == b.refine_compile_cmd("x")[:-2] == b.refine_grad_compile_cmd("x")[:-2]
    assert os.path.basename(b.REFINE_ROBUST_OUT) == "libcvxpnpl_amd_refine_robust.so"


def _calls(G):
    from cvxpnpl_amd import _lib

    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it reads or launches anything
    good = _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), 30, 1e-10, 1e-3, _lib.LOSS_HUBER, 1.0)

    def batch(fn, B=2, n_p=10, p2=p, p3=p, n_l=6, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=1, mp=None, ml=None, wp=None, wl=None,
              o=good, oR=p, ot=p, cost=p, iters=p, ost=p, n_live=p, rw=None, n_in=p, last=None):
        return fn(B, n_p, p2, p3, n_l, l2, l3, K, per, R, t, st, stride, admit, mp, ml, wp, wl, C.byref(o) if o is not None else None, oR, ot, cost, iters,
                  ost, n_live, rw, n_in, last)

    def scenes(F=2, op=p, n_pts=10, ol=p, n_lines=6, p2=p, p3=p, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=1, mp=None, ml=None,
               wp=None, wl=None, o=good, oR=p, ot=p, cost=p, iters=p, ost=p, n_live=p, rwp=None, rwl=None, n_in=p):
        return G.cvxpnpl_refine_robust_scenes(F, op, n_pts, ol, n_lines, p2, p3, l2, l3, K, per, R, t, st, stride, admit, mp, ml, wp, wl,
                                              C.byref(o) if o is not None else None, oR, ot, cost, iters, ost, n_live, rwp, rwl, n_in, None)

    return p, batch, scenes


def _opts(**kw):
    from cvxpnpl_amd import _lib

    f = dict(struct_size=C.sizeof(_lib.RefineRobustOpts), max_iters=30, step_tol=1e-10, lambda0=1e-3, loss=_lib.LOSS_HUBER, scale_px=1.0)
    f.update(kw)
    return _lib.RefineRobustOpts(*(f[k] for k in ("struct_size", "max_iters", "step_tol", "lambda0", "loss", "scale_px")))


def test_bad_arguments_are_rejected_without_gpu(G):
    p, batch, scenes = _calls(G)
    err = G.cvxpnpl_refine_robust_last_error
    bad_opts = ((_opts(struct_size=32), b"struct_size"), (_opts(max_iters=-1), b"max_iters"), (_opts(step_tol=float("nan")), b"step_tol"),
                (_opts(lambda0=-1.0), b"lambda0"), (_opts(loss=3), b"loss"), (_opts(loss=-1), b"loss"), (_opts(scale_px=0.0), b"scale_px"),
                (_opts(scale_px=-2.0), b"scale_px"), (_opts(scale_px=float("inf")), b"scale_px"), (_opts(scale_px=float("nan")), b"scale_px"),
                (_opts(loss=2, scale_px=0.0), b"scale_px"))
    for fn, name, last in ((G.cvxpnpl_refine_robust_batch, b"cvxpnpl_refine_robust_batch:", None),
                           (G.cvxpnpl_refine_robust_batch_host, b"cvxpnpl_refine_robust_batch_host:", 1)):
        def run(**kw):
            return batch(fn, last=last, **kw)

        assert run(B=-1) == -1 and err().startswith(name) and b"bad arguments" in err()
        assert run(n_p=-1) == -1 and run(n_l=-2) == -1
        assert run(p2=None) == -1 and b"correspondence pointer" in err()
        assert run(l3=None) == -1 and run(p3=None) == -1 and run(l2=None) == -1
        assert run(K=None) == -1 and run(R=None) == -1 and run(t=None) == -1
        assert run(per=2) == -1 and run(per=-1) == -1 and b"0 or 1" in err()
        for out in ("oR", "ot", "cost", "iters", "ost", "n_live", "n_in"):
            assert run(**{out: None}) == -1 and b"output pointer" in err(), out
        assert run(st=p, stride=-1) == -1 and b"status_stride" in err()
        for o, what in bad_opts:
            assert run(o=o) == -1 and what in err(), what
        z = None                                                                            # a zero-size call is a no-op whatever the pointers
        assert run(B=0, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, oR=z, ot=z, cost=z, iters=z, ost=z, n_live=z, n_in=z, per=7, o=_opts(loss=9)) == 0
    assert scenes(F=-1) == -1 and err().startswith(b"cvxpnpl_refine_robust_scenes:")
    assert scenes(n_pts=-1) == -1 and scenes(n_lines=-1) == -1
    assert scenes(op=None) == -1 and scenes(ol=None) == -1 and b"offsets" in err()
    assert scenes(p3=None) == -1 and scenes(l2=None) == -1 and scenes(K=None) == -1 and scenes(R=None) == -1 and scenes(t=None) == -1
    assert scenes(per=3) == -1 and scenes(n_in=None) == -1 and scenes(st=p, stride=-2) == -1
    for o, what in bad_opts:
        assert scenes(o=o) == -1 and what in err(), what
    z = None
    assert scenes(F=0, op=z, ol=z, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, oR=z, ot=z, cost=z, iters=z, ost=z, n_live=z, n_in=z, n_pts=0, n_lines=0) == 0


def test_l2_ignores_scale_px(G):
    p, batch, _ = _calls(G)
    assert batch(G.cvxpnpl_refine_robust_batch_host, last=1, K=None, o=_opts(loss=0, scale_px=float("nan"))) == -1
    assert b"K, R or t" in G.cvxpnpl_refine_robust_last_error()                             # (the options passed: the next check spoke)


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.REFINE_ROBUST_RESOURCES) and os.path.getmtime(b.REFINE_ROBUST_RESOURCES) >= os.path.getmtime(b.REFINE_ROBUST_OUT) - 1
    table = b.kernel_resources(b.REFINE_ROBUST_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = []
    for name, g in golden.items():
        r = table[name]
        for k in ("occupancy", "lds", "scratch", "sgpr_spill", "vgpr_spill"):
            if r[k] != g[k]:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]}")
        for k in ("vgpr", "agpr"):
            if r[k] > g[k] + REG_SLACK:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]} (+{REG_SLACK} allowed)")
        if g["scratch"] or g["vgpr_spill"] or g["sgpr_spill"] or r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]:
            problems.append(f"{name}: scratch or spills")
    assert not problems, "\n".join(problems)


def test_python_entry_points_validate_before_they_ask_for_a_gpu():
    """Every ValueError below is raised before _require_gpu: this test runs on a machine without a GPU."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import refine_robust as rb

    for name in ("refine_pose_batch_robust", "refine_scenes_robust", "refine_pose_batch_robust_host", "RobustRefineResult"):
        assert getattr(ca, name) is getattr(rb, name)
    B = 3
    R, t = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1), torch.zeros(B, 3, dtype=torch.float64)
    p2, p3, K = torch.zeros(B, 5, 2, dtype=torch.float64), torch.zeros(B, 5, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    w = torch.ones(B, 5, dtype=torch.float64)
    good = dict(R=R, t=t, pts_2d=p2, pts_3d=p3, K=K, weights_pts=w)
    with pytest.raises(ValueError, match="no CPU path"):
        rb.refine_pose_batch_robust(**good)
    meta = torch.device("meta")
    wide = torch.ones(B, 10, dtype=torch.float64)
    for bad, match in ((dict(loss="tukey"), "loss"), (dict(loss=1), "loss"), (dict(scale_px=0.0), "scale_px"), (dict(scale_px=-1.0), "scale_px"),
                       (dict(scale_px=float("nan")), "scale_px"), (dict(scale_px=float("inf")), "scale_px"), (dict(scale_px="wide"), "scale_px"),
                       (dict(loss="cauchy", scale_px=0.0), "scale_px"),
                       (dict(weights_pts=w.float()), "weights_pts: dtype"), (dict(weights_pts=w[:, :4]), "weights_pts: shape"),
                       (dict(weights_pts=w.to(meta)), "weights_pts: on meta"), (dict(weights_pts=wide[:, ::2]), "weights_pts: not contiguous"),
                       (dict(weights_pts=w.numpy()), "weights_pts: expected a torch tensor"), (dict(weights_lines=w), "weights_lines: shape"),
                       (dict(R=R.numpy()), "torch tensor"), (dict(t=t.float()), "dtype"), (dict(pts_2d=None), "go together"),
                       (dict(pts_2d=None, pts_3d=None), "at least one"), (dict(K=K[:2]), "K must be"),
                       (dict(status=torch.zeros(B, dtype=torch.int64)), "status"), (dict(mask_pts=torch.ones(B, 5, dtype=torch.bool)), "dtype"),
                       (dict(max_iters=-1), "max_iters"), (dict(step_tol=-1.0), "step_tol")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            rb.refine_pose_batch_robust(**kw)
    with pytest.raises(ValueError, match="no CPU path"):                                  # l2 does not look at scale_px
        rb.refine_pose_batch_robust(**dict(good, loss="l2", scale_px=-1.0))
    with pytest.raises(ValueError, match="loss"):                                          # the options are checked before the scenes
        rb.refine_scenes_robust(object(), R, t, loss="l1")
    with pytest.raises(ValueError, match="scale_px"):
        rb.refine_scenes_robust(object(), R, t, scale_px=0.0)
    with pytest.raises(ValueError, match="ransac.Scenes"):
        rb.refine_scenes_robust(object(), R, t)
    host = dict(R=np.eye(3)[None], t=np.zeros((1, 3)), pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(3))
    for bad, match in ((dict(loss="l1"), "loss"), (dict(scale_px=0.0), "scale_px"), (dict(weights_pts=np.ones((1, 4), np.float32)), "float64"),
                       (dict(weights_pts=np.ones((1, 5))), "shape"), (dict(weights_pts=np.ones((2, 8))[:1, ::2]), "contiguous"),
                       (dict(weights_pts=[[1.0] * 4]), "float64 numpy"), (dict(K=np.eye(4)), "K must be"), (dict(t=np.zeros((2, 3))), "t: expected")):
        with pytest.raises(ValueError, match=match):
            rb.refine_pose_batch_robust_host(**dict(host, **bad))


def test_host_path_is_clean_under_asan_and_ubsan_in_a_stand_alone_program(tmp_path):
    """cvxpnpl_refine_robust_batch_host compiled from source with -fsanitize=address,undefined into a program of its own (no Python, nothing
    preloaded): n_p = 0, n_l = 0, 65 records with masks and weights, a null robust_w, a strided status column, guard words around every
    output."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for rt in ("libasan.a", "libubsan.a"):      # linked statically: the program carries its runtimes and needs nothing from its environment
        path = subprocess.run(["g++", f"-print-file-name={rt}"], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip(f"{rt} not installed")
    exe = str(tmp_path / "refine_robust_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread",
           "-o", exe,
           os.path.join(ROOT, "tests", "hostsim", "refine_robust_sanitize_main.cpp"), os.path.join(ROOT, "cvxpnpl_amd", "csrc", "host_refine_robust.cpp")]
    c = subprocess.run(cmd, capture_output=True, text=True)
    if c.returncode != 0 and "sanitize" in c.stderr and "cannot find" in c.stderr:
        pytest.skip("the sanitizer runtimes do not link here")
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and "ok" in p.stdout, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
