"""The twelfth library (libcvxpnpl_amd_refine_robust_auto.so, include/cvxpnpl_amd_refine_robust_auto.h): it builds by cross-compilation,
exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels free of scratch and
spills (tests/golden/refine_robust_auto_kernel_resources.json; the loop kernels within the seventh library's registers) and leaves the
other eleven libraries' compile commands alone; the host-side validation of the Python entry points; and the host path compiled from
source under ASan + UBSan in a stand-alone program (tests/hostsim/refine_robust_auto_sanitize_main.cpp).  No GPU needed."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refine_robust_auto_kernel_resources.json")
GOLDEN_SEVENTH = os.path.join(ROOT, "tests", "golden", "refine_robust_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_refine_library.py); occupancy, LDS, scratch and spills are exact
LOOP_KERNELS = {"cvxra::refine_robust_pp_group_kernel<1>": "cvxrb::refine_robust_group_kernel<1>",
                "cvxra::refine_robust_pp_group_kernel<2>": "cvxrb::refine_robust_group_kernel<2>",
                "cvxra::refine_robust_pp_group_kernel<4>": "cvxrb::refine_robust_group_kernel<4>",
                "cvxra::refine_robust_pp_group_kernel<0>": "cvxrb::refine_robust_group_kernel<0>",
                "cvxra::refine_robust_pp_scenes_kernel": "cvxrb::refine_robust_scenes_kernel",
                "cvxra::robust_w_pp_group_kernel": "cvxrb::robust_w_group_kernel", "cvxra::robust_w_pp_scenes_kernel": "cvxrb::robust_w_scenes_kernel"}
KERNELS = tuple(LOOP_KERNELS) + ("cvxra::robust_scale_group_kernel<1>", "cvxra::robust_scale_group_kernel<2>", "cvxra::robust_scale_group_kernel<4>",
                                 "cvxra::robust_scale_group_kernel<0>", "cvxra::robust_scale_scenes_kernel", "cvxra::robust_cov_group_kernel",
                                 "cvxra::robust_cov_scenes_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_refine_robust_auto()
    assert os.path.exists(build.REFINE_ROBUST_AUTO_OUT)
    return _lib.refine_robust_auto_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_refine_robust_auto.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.REFINE_ROBUST_AUTO_EXPORTS), declared ^ set(_lib.REFINE_ROBUST_AUTO_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.REFINE_ROBUST_AUTO_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared
    assert not [ln for ln in nm.splitlines() if re.search(r"err_buf|bad_args|launched|check_\w+|host_problem|host_weights|host_grads|fill_batch|fill_scenes|for_chunks", ln)], "the shared argument checks are exported"
    assert G.cvxpnpl_refine_robust_auto_version().startswith(b"cvxpnpl_amd_refine_robust_auto")
    assert _lib.RefineRobustAutoOpts is _lib.RefineRobustOpts and C.sizeof(_lib.RefineRobustAutoOpts) == 40


def test_the_other_eleven_compile_commands_are_unchanged_and_the_new_one_has_the_grad_flags():
    from cvxpnpl_amd import build as b

    flags = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value"]
    assert b.compile_cmd("x")[1:] == flags + ["-mllvm", "-enable-ipra=0", "-o", "x", b.SRC, b.LANE_SRC, b.HOST_SRC]
    assert b.grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.GRAD_SRC, b.GRAD_HOST_SRC]
    assert b.ransac_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_SRC]
    assert b.ransac_pnpl_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_PNPL_SRC]
    assert b.refine_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_SRC, b.REFINE_HOST_SRC]
    assert b.refine_grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_GRAD_SRC, b.REFINE_GRAD_HOST_SRC]
    assert b.refine_robust_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_ROBUST_SRC, b.REFINE_ROBUST_HOST_SRC]
    assert b.refine_robust_grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_ROBUST_GRAD_SRC, b.REFINE_ROBUST_GRAD_HOST_SRC]
    assert b.ransac_adaptive_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_ADAPTIVE_SRC]
    assert b.ransac_guided_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_GUIDED_SRC]
    assert b.ransac_pnpl_adaptive_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_PNPL_ADAPTIVE_SRC]
    assert b.refine_robust_auto_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_ROBUST_AUTO_SRC, b.REFINE_ROBUST_AUTO_HOST_SRC]
    assert b.refine_robust_auto_compile_cmd("x")[:-2] == b.refine_robust_compile_cmd("x")[:-2] == b.refine_robust_grad_compile_cmd("x")[:-2]
    assert os.path.basename(b.REFINE_ROBUST_AUTO_OUT) == "libcvxpnpl_amd_refine_robust_auto.so"


def _opts(**kw):
    from cvxpnpl_amd import _lib

    f = dict(struct_size=C.sizeof(_lib.RefineRobustOpts), max_iters=30, step_tol=1e-10, lambda0=1e-3, loss=_lib.LOSS_HUBER, scale_px=1.0)
    f.update(kw)
    return _lib.RefineRobustOpts(*(f[k] for k in ("struct_size", "max_iters", "step_tol", "lambda0", "loss", "scale_px")))


P = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it reads or launches anything


def _batch_head(B=2, n_p=10, p2=P, p3=P, n_l=6, l2=P, l3=P, **_):
    return [B, n_p, p2, p3, n_l, l2, l3]


def _scenes_head(B=2, op=P, n_pts=10, ol=P, n_lines=6, p2=P, p3=P, l2=P, l3=P, **_):
    return [B, op, n_pts, ol, n_lines, p2, p3, l2, l3]


def _pose(K=P, per=0, R=P, t=P, st=None, stride=1, admit=1, **_):
    return [K, per, R, t, st, stride, admit, None, None, None, None]


def _scale_call(fn, head, last, **kw):
    o = dict(sigma=P, med=P, n_live=P, ost=P, sq=P, sq_l=P)
    o.update({k: v for k, v in kw.items() if k in o})
    tail = [o["sigma"], o["med"], o["n_live"], o["ost"], o["sq"]] + ([o["sq_l"]] if head is _scenes_head else [])
    return fn(*head(**kw), *_pose(**kw), *tail, last)


def _loop_call(fn, head, last, o="good", **kw):
    out = dict(oR=P, ot=P, cost=P, iters=P, ost=P, n_live=P, n_in=P)
    out.update({k: v for k, v in kw.items() if k in out})
    opts = _opts() if o == "good" else o
    tail = [None] + ([None] if head is _scenes_head else [])
    return fn(*head(**kw), *_pose(**kw), kw.get("scale"), C.byref(opts) if opts is not None else None, out["oR"], out["ot"], out["cost"], out["iters"],
              out["ost"], out["n_live"], *tail, out["n_in"], last)


def _cov_call(fn, head, last, loss=1, scale_px=1.0, **kw):
    out = dict(cov=P, cst=P)
    out.update({k: v for k, v in kw.items() if k in out})
    K, per, R, t = _pose(**kw)[:4]
    return fn(*head(**kw), K, per, R, t, None, None, None, None, None, loss, scale_px, kw.get("scale"), out["cov"], out["cst"], last)


def test_bad_arguments_are_rejected_without_gpu(G):
    err = G.cvxpnpl_refine_robust_auto_last_error
    z = None
    zeros_b = dict(p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, per=7)
    families = ((_scale_call, G.cvxpnpl_robust_scale_batch, G.cvxpnpl_robust_scale_batch_host, G.cvxpnpl_robust_scale_scenes, ("sigma", "med", "n_live", "ost", "sq")),
                (_loop_call, G.cvxpnpl_refine_robust_pp_batch, G.cvxpnpl_refine_robust_pp_batch_host, G.cvxpnpl_refine_robust_pp_scenes,
                 ("oR", "ot", "cost", "iters", "ost", "n_live", "n_in")),
                (_cov_call, G.cvxpnpl_robust_cov_batch, G.cvxpnpl_robust_cov_batch_host, G.cvxpnpl_robust_cov_scenes, ("cov", "cst")))
    for call, dev, host, scenes, outs in families:
        for fn, last in ((dev, None), (host, 1)):
            def run(**kw):
                return call(fn, _batch_head, last, **kw)

            name = fn.__name__.encode() + b":"
            assert run(B=-1) == -1 and err().startswith(name) and b"bad arguments" in err()
            assert run(n_p=-1) == -1 and run(n_l=-2) == -1
            assert run(p2=None) == -1 and b"correspondence pointer" in err()
            assert run(l3=None) == -1 and run(p3=None) == -1 and run(l2=None) == -1
            assert run(K=None) == -1 and run(R=None) == -1 and run(t=None) == -1
            assert run(per=2) == -1 and run(per=-1) == -1 and b"0 or 1" in err()
            for out in outs:
                assert run(**{out: None}) == -1 and b"output pointer" in err(), out
            if call is not _cov_call:
                assert run(st=P, stride=-1) == -1 and b"status_stride" in err()
            assert run(B=0, **zeros_b, **{out: z for out in outs}) == 0             # a zero-size call is a no-op whatever the pointers

        def srun(**kw):
            return call(scenes, _scenes_head, None, **kw)

        assert srun(B=-1) == -1 and err().startswith(scenes.__name__.encode() + b":")
        assert srun(n_pts=-1) == -1 and srun(n_lines=-1) == -1
        assert srun(op=None) == -1 and srun(ol=None) == -1 and b"offsets" in err()
        assert srun(p3=None) == -1 and srun(l2=None) == -1 and srun(K=None) == -1 and srun(R=None) == -1 and srun(t=None) == -1
        assert srun(per=3) == -1 and srun(**{outs[-1]: None}) == -1
        assert srun(B=0, op=z, ol=z, n_pts=0, n_lines=0, **zeros_b, **{out: z for out in outs}) == 0
    assert _scale_call(G.cvxpnpl_robust_scale_scenes, _scenes_head, None, sq_l=None) == -1 and b"workspace" in err()
    bad_opts = ((_opts(struct_size=32), b"struct_size"), (_opts(max_iters=-1), b"max_iters"), (_opts(step_tol=float("nan")), b"step_tol"),
                (_opts(lambda0=-1.0), b"lambda0"), (_opts(loss=3), b"loss"), (_opts(loss=-1), b"loss"), (_opts(scale_px=0.0), b"scale_px"),
                (_opts(scale_px=float("inf")), b"scale_px"), (_opts(loss=2, scale_px=float("nan")), b"scale_px"))
    for fn, head, last in ((G.cvxpnpl_refine_robust_pp_batch, _batch_head, None), (G.cvxpnpl_refine_robust_pp_batch_host, _batch_head, 1),
                           (G.cvxpnpl_refine_robust_pp_scenes, _scenes_head, None)):
        for o, what in bad_opts:
            assert _loop_call(fn, head, last, o=o) == -1 and what in err(), what
    for fn, head, last in ((G.cvxpnpl_robust_cov_batch, _batch_head, None), (G.cvxpnpl_robust_cov_batch_host, _batch_head, 1), (G.cvxpnpl_robust_cov_scenes, _scenes_head, None)):
        assert _cov_call(fn, head, last, loss=3) == -1 and b"loss" in err()
        assert _cov_call(fn, head, last, scale_px=0.0) == -1 and b"scale_px" in err()
        assert _cov_call(fn, head, last, scale_px=float("nan"), loss=2) == -1 and b"scale_px" in err()
        assert _cov_call(fn, head, last, scale_px=0.0, scale=P, K=None) == -1 and b"K, R or t" in err()   # a per-problem scale: the uniform one is not looked at
        assert _cov_call(fn, head, last, scale_px=-1.0, loss=0, K=None) == -1 and b"K, R or t" in err()   # nor under l2


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.REFINE_ROBUST_AUTO_RESOURCES) and os.path.getmtime(b.REFINE_ROBUST_AUTO_RESOURCES) >= os.path.getmtime(b.REFINE_ROBUST_AUTO_OUT) - 1
    table = {k: v for k, v in b.kernel_resources(b.REFINE_ROBUST_AUTO_RESOURCES).items() if k.startswith("cvxra::")}  # (the seventh's non-template kernels ride along: csrc/refine_robust_auto_kernel.h)
    golden = json.load(open(GOLDEN))
    seventh = json.load(open(GOLDEN_SEVENTH))
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
        if name in LOOP_KERNELS:                                                          # the seventh library's kernel with one more load
            s = seventh[LOOP_KERNELS[name]]
            for k in ("vgpr", "agpr"):
                if r[k] > s[k] + REG_SLACK:
                    problems.append(f"{name}: {k} {r[k]}, the seventh library's kernel has {s[k]} (+{REG_SLACK} allowed)")
            if r["occupancy"] != s["occupancy"] or r["lds"] != s["lds"]:
                problems.append(f"{name}: occupancy / LDS differ from the seventh library's kernel")
    assert not problems, "\n".join(problems)


def test_python_entry_points_validate_before_they_ask_for_a_gpu():
    """Every ValueError below is raised before _require_gpu: this test runs on a machine without a GPU."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import refine_robust_auto as ra

    for name in ra.__all__:
        if name != "SCALE_FACTOR_95":
            assert getattr(ca, name) is getattr(ra, name), name
    assert ra.SCALE_FACTOR_95 == np.sqrt(-2.0 * np.log(0.05))
    B = 3
    R, t = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1), torch.zeros(B, 3, dtype=torch.float64)
    p2, p3, K = torch.zeros(B, 5, 2, dtype=torch.float64), torch.zeros(B, 5, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    w = torch.ones(B, 5, dtype=torch.float64)
    sc = torch.ones(B, dtype=torch.float64)
    good = dict(R=R, t=t, pts_2d=p2, pts_3d=p3, K=K, weights_pts=w)
    for fn in (ra.refine_pose_batch_robust_auto, ra.robust_scale_batch, ra.robust_covariance_batch):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(**good)
    with pytest.raises(ValueError, match="no CPU path"):
        ra.refine_pose_batch_robust_auto(**good, scale_px=sc)
    meta = torch.device("meta")
    wide = torch.ones(B, 2, dtype=torch.float64)
    scale_bad = ((dict(scale_px=sc.float()), "scale_px: dtype"), (dict(scale_px=sc[:2]), "scale_px: shape"), (dict(scale_px=sc.to(meta)), "scale_px: on meta"),
                 (dict(scale_px=wide[:, 0]), "scale_px: not contiguous"), (dict(scale_px=sc.numpy()), "scale_px: expected"), (dict(scale_px=0.0), "scale_px"),
                 (dict(scale_px=float("nan")), "scale_px"), (dict(scale_px="wide"), "scale_px"), (dict(loss="tukey"), "loss"))
    common = ((dict(weights_pts=w.float()), "weights_pts: dtype"), (dict(R=R.numpy()), "torch tensor"), (dict(pts_2d=None), "go together"),
              (dict(K=K[:2]), "K must be"), (dict(mask_pts=torch.ones(B, 5, dtype=torch.bool)), "dtype"))
    auto_bad = ((dict(scale_factor=0.0), "scale_factor"), (dict(scale_factor=float("inf")), "scale_factor"), (dict(scale_factor="x"), "scale_factor"),
                (dict(scale_floor_px=-1.0), "scale_floor_px"), (dict(scale_floor_px=float("nan")), "scale_floor_px"), (dict(scale_rounds=0), "scale_rounds"),
                (dict(scale_rounds=5), "scale_rounds"), (dict(scale_rounds=1.5), "scale_rounds"), (dict(max_iters=-1), "max_iters"),
                (dict(step_tol=-1.0), "step_tol"), (dict(status=torch.zeros(B, dtype=torch.int64)), "status"))
    for fn, cases in ((ra.refine_pose_batch_robust_auto, scale_bad + common + auto_bad), (ra.robust_covariance_batch, scale_bad + common),
                      (ra.robust_scale_batch, common)):
        for bad, match in cases:
            with pytest.raises(ValueError, match=match):
                fn(**dict(good, **bad))
    with pytest.raises(ValueError, match="status"):
        ra.robust_covariance_batch(**good, status=torch.zeros(B, 2, dtype=torch.int32)[:, 0])
    with pytest.raises(ValueError, match="no CPU path"):                                  # l2 does not look at a float scale
        ra.refine_pose_batch_robust_auto(**dict(good, loss="l2", scale_px=-1.0))
    for fn in (ra.refine_scenes_robust_auto, ra.robust_covariance_scenes):
        with pytest.raises(ValueError, match="loss"):                                      # the options are checked before the scenes
            fn(object(), R, t, loss="l1")
        with pytest.raises(ValueError, match="scale_px"):
            fn(object(), R, t, scale_px=0.0)
        with pytest.raises(ValueError, match="ransac.Scenes"):
            fn(object(), R, t)
    with pytest.raises(ValueError, match="scale_rounds"):
        ra.refine_scenes_robust_auto(object(), R, t, scale_rounds=9)
    with pytest.raises(ValueError, match="ransac.Scenes"):
        ra.robust_scale_scenes(object(), R, t)
    host = dict(R=np.eye(3)[None], t=np.zeros((1, 3)), pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(3))
    for bad, match in ((dict(loss="l1"), "loss"), (dict(scale_px=0.0), "scale_px"), (dict(scale_px=np.ones(2)), "scale_px"),
                       (dict(scale_px=np.ones(1, np.float32)), "scale_px"), (dict(scale_px=torch.ones(1, dtype=torch.float64)), "scale_px"),
                       (dict(scale_rounds=0), "scale_rounds"), (dict(scale_factor=-2.0), "scale_factor"), (dict(weights_pts=np.ones((1, 5))), "shape"),
                       (dict(K=np.eye(4)), "K must be")):
        with pytest.raises(ValueError, match=match):
            ra.refine_pose_batch_robust_auto_host(**dict(host, **bad))
    with pytest.raises(ValueError, match="scale_px"):
        ra.robust_covariance_host(**host, scale_px=np.ones(3))
    with pytest.raises(ValueError, match="t: expected"):
        ra.robust_scale_batch_host(**dict(host, t=np.zeros((2, 3))))


def test_host_path_is_clean_under_asan_and_ubsan_in_a_stand_alone_program(tmp_path):
    """The three host entry points compiled from source with -fsanitize=address,undefined into a program of its own (no Python, nothing
    preloaded): ties, no points, no lines, no live record, 65 records with masks and weights, bad scale elements, a strided status column,
    a zero batch; guard words around every output."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for rt in ("libasan.a", "libubsan.a"):      # linked statically: the program carries its runtimes and needs nothing from its environment
        path = subprocess.run(["g++", f"-print-file-name={rt}"], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip(f"{rt} not installed")
    exe = str(tmp_path / "refine_robust_auto_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread",
           "-o", exe,
           os.path.join(ROOT, "tests", "hostsim", "refine_robust_auto_sanitize_main.cpp"), os.path.join(ROOT, "cvxpnpl_amd", "csrc", "host_refine_robust_auto.cpp")]
    c = subprocess.run(cmd, capture_output=True, text=True)
    if c.returncode != 0 and "sanitize" in c.stderr and "cannot find" in c.stderr:
        pytest.skip("the sanitizer runtimes do not link here")
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and "ok" in p.stdout, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
