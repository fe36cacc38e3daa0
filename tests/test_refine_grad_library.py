"""The library of the refinement's backward pass (libcvxpnpl_amd_refine_grad.so, include/cvxpnpl_amd_refine_grad.h): it builds by
cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels
free of scratch and spills (tests/golden/refine_grad_kernel_resources.json) and leaves the other five libraries' compile commands alone;
the host-side validation of the Python entry points; and the host path compiled from source under ASan + UBSan in a stand-alone program
(tests/hostsim/refine_vjp_sanitize_main.cpp).  No GPU needed."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refine_grad_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_refine_library.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxrg::refine_vjp_group_kernel<1>", "cvxrg::refine_vjp_group_kernel<2>", "cvxrg::refine_vjp_group_kernel<4>",
           "cvxrg::refine_vjp_group_kernel<0>", "cvxrg::refine_vjp_scenes_kernel")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_refine_grad()
    assert os.path.exists(build.REFINE_GRAD_OUT)
    return _lib.refine_grad_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_refine_grad.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.REFINE_GRAD_EXPORTS), declared ^ set(_lib.REFINE_GRAD_EXPORTS)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.REFINE_GRAD_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared
    assert not [ln for ln in nm.splitlines() if re.search(r"err_buf|bad_args|launched|check_\w+|host_problem|host_weights|host_grads|fill_batch|fill_scenes|for_chunks", ln)], "the shared argument checks are exported"
    assert G.cvxpnpl_refine_grad_version().startswith(b"cvxpnpl_amd_refine_grad")


def test_the_other_compile_commands_are_unchanged_and_the_new_one_has_the_grad_flags():
    from cvxpnpl_amd import build as b

    flags = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value"]
    assert b.compile_cmd("x")[1:] == flags + ["-mllvm", "-enable-ipra=0", "-o", "x", b.SRC, b.LANE_SRC, b.HOST_SRC]
    assert b.grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.GRAD_SRC, b.GRAD_HOST_SRC]
    assert b.ransac_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_SRC]
    assert b.ransac_pnpl_compile_cmd("x")[1:] == flags + ["-o", "x", b.RANSAC_PNPL_SRC]
    assert b.refine_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_SRC, b.REFINE_HOST_SRC]
    assert b.refine_grad_compile_cmd("x")[1:] == flags + ["-o", "x", b.REFINE_GRAD_SRC, b.REFINE_GRAD_HOST_SRC]
    assert b.refine_grad_compile_cmd("x")[:-2] == b.grad_compile_cmd("x")[:-2]                     # the grad library's flags, exactly
    assert os.path.basename(b.REFINE_GRAD_OUT) == "libcvxpnpl_amd_refine_grad.so"


def _calls(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it reads or launches anything

    def batch(fn, B=2, n_p=10, p2=p, p3=p, n_l=6, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=1, mp=None, ml=None, gR=p, gt=p,
              g2=p, g3=p, h2=p, h3=p, vst=p, info=None, last=None):
        return fn(B, n_p, p2, p3, n_l, l2, l3, K, per, R, t, st, stride, admit, mp, ml, gR, gt, g2, g3, h2, h3, vst, info, last)

    def scenes(F=2, op=p, n_pts=10, ol=p, n_lines=6, p2=p, p3=p, l2=p, l3=p, K=p, per=0, R=p, t=p, st=None, stride=1, admit=1, mp=None, ml=None,
               gR=p, gt=p, g2=p, g3=p, h2=p, h3=p, vst=p, info=None):
        return G.cvxpnpl_refine_vjp_scenes(F, op, n_pts, ol, n_lines, p2, p3, l2, l3, K, per, R, t, st, stride, admit, mp, ml, gR, gt, g2, g3, h2, h3,
                                           vst, info, None)

    return p, batch, scenes


def test_bad_arguments_are_rejected_without_gpu(G):
    p, batch, scenes = _calls(G)
    err = G.cvxpnpl_refine_grad_last_error
    for fn, name, last in ((G.cvxpnpl_refine_vjp_batch, b"cvxpnpl_refine_vjp_batch:", None),
                           (G.cvxpnpl_refine_vjp_batch_host, b"cvxpnpl_refine_vjp_batch_host:", 1)):
        def run(**kw):
            return batch(fn, last=last, **kw)

        assert run(B=-1) == -1 and err().startswith(name) and b"bad arguments" in err()
        assert run(n_p=-1) == -1 and run(n_l=-2) == -1
        assert run(p2=None) == -1 and b"correspondence pointer" in err()
        assert run(l3=None) == -1 and run(p3=None) == -1 and run(l2=None) == -1
        assert run(K=None) == -1 and run(R=None) == -1 and run(t=None) == -1
        assert run(per=2) == -1 and run(per=-1) == -1 and b"0 or 1" in err()
        assert run(vst=None) == -1 and b"vjp_status" in err()
        assert run(st=p, stride=-1) == -1 and b"status_stride" in err()
        z = None                                                                            # a zero-size call is a no-op whatever the pointers
        assert run(B=0, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, gR=z, gt=z, g2=z, g3=z, h2=z, h3=z, vst=z, per=7) == 0
    assert scenes(F=-1) == -1 and err().startswith(b"cvxpnpl_refine_vjp_scenes:")
    assert scenes(n_pts=-1) == -1 and scenes(n_lines=-1) == -1
    assert scenes(op=None) == -1 and scenes(ol=None) == -1 and b"offsets" in err()
    assert scenes(p3=None) == -1 and scenes(l2=None) == -1 and scenes(K=None) == -1 and scenes(R=None) == -1 and scenes(t=None) == -1
    assert scenes(per=3) == -1 and scenes(vst=None) == -1 and scenes(st=p, stride=-2) == -1
    z = None
    assert scenes(F=0, op=z, ol=z, p2=z, p3=z, l2=z, l3=z, K=z, R=z, t=z, gR=z, gt=z, g2=z, g3=z, h2=z, h3=z, vst=z, n_pts=0, n_lines=0) == 0


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.REFINE_GRAD_RESOURCES) and os.path.getmtime(b.REFINE_GRAD_RESOURCES) >= os.path.getmtime(b.REFINE_GRAD_OUT) - 1
    table = b.kernel_resources(b.REFINE_GRAD_RESOURCES)
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
    from cvxpnpl_amd import refine_grad as rg

    for name in ("refine_vjp", "refine_vjp_scenes", "refine_vjp_host", "refine_pose_batch_diff", "pose_passthrough"):
        assert getattr(ca, name) is getattr(rg, name)
    B = 3
    R, t = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1), torch.zeros(B, 3, dtype=torch.float64)
    p2, p3, K = torch.zeros(B, 5, 2, dtype=torch.float64), torch.zeros(B, 5, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    st = torch.zeros(B, dtype=torch.int32)
    good = dict(R=R, t=t, status=st, grad_R=R.clone(), grad_t=t.clone(), pts_2d=p2, pts_3d=p3, K=K)
    with pytest.raises(ValueError, match="no CPU path"):
        rg.refine_vjp(**good)
    meta = torch.device("meta")
    for bad, match in ((dict(R=R.numpy()), "torch tensor"), (dict(t=t.float()), "dtype"), (dict(t=t[:, :2]), "shape"), (dict(t=t.to(meta)), "on meta"),
                       (dict(grad_R=R[:2]), "grad_R"), (dict(grad_t=t.float()), "grad_t"), (dict(pts_2d=p2[:, :4]), "shape"),
                       (dict(pts_2d=None), "go together"), (dict(pts_2d=None, pts_3d=None), "at least one"), (dict(K=K[:2]), "K must be"),
                       (dict(status=torch.zeros(B, dtype=torch.int64)), "status"), (dict(mask_pts=torch.ones(B, 5, dtype=torch.bool)), "dtype"),
                       (dict(mask_pts=torch.ones(B, 4, dtype=torch.uint8)), "shape"), (dict(want=("pts_2d", "K")), "want"),
                       (dict(admit_mask=-1), "admit_mask")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            rg.refine_vjp(**kw)
    with pytest.raises(ValueError, match="ransac.Scenes"):
        rg.refine_vjp_scenes(object(), R, t, st)
    with pytest.raises(ValueError, match="want"):
        rg.refine_vjp_scenes(object(), R, t, st, want=("nothing",))
    with pytest.raises(ValueError, match="no CPU path"):                                  # the autograd form validates through refine_pose_batch
        rg.refine_pose_batch_diff(R, t, pts_2d=p2.requires_grad_(True), pts_3d=p3, K=K)
    with pytest.raises(ValueError, match="max_iters"):
        rg.refine_pose_batch_diff(R, t, pts_2d=p2, pts_3d=p3, K=K, max_iters=-1)
    with pytest.raises(ValueError, match="admit_mask"):
        rg.refine_pose_batch_diff(R, t, pts_2d=p2, pts_3d=p3, K=K, admit_mask=1 << 40)
    with pytest.raises(ValueError):                                                      # the host form checks shapes too
        rg.refine_vjp_host(np.eye(3)[None], np.zeros((2, 3)), None, pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(3))
    with pytest.raises(ValueError, match="K must be"):
        rg.refine_vjp_host(np.eye(3)[None], np.zeros((1, 3)), None, pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)), K=np.eye(4))
    with pytest.raises(ValueError, match="grad_R"):
        rg.refine_vjp_host(np.eye(3)[None], np.zeros((1, 3)), None, grad_R=np.zeros((2, 3, 3)), pts_2d=np.zeros((1, 4, 2)), pts_3d=np.zeros((1, 4, 3)),
                           K=np.eye(3))


def test_host_path_is_clean_under_asan_and_ubsan_in_a_stand_alone_program(tmp_path):
    """cvxpnpl_refine_vjp_batch_host compiled from source with -fsanitize=address,undefined into a program of its own (no Python, nothing
    preloaded): n_p = 0, n_l = 0, 65 records with masks, null gradient pointers, a strided status column."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for rt in ("libasan.a", "libubsan.a"):      # linked statically: the program carries its runtimes and needs nothing from its environment
        path = subprocess.run(["g++", f"-print-file-name={rt}"], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip(f"{rt} not installed")
    exe = str(tmp_path / "refine_vjp_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread",
           "-o", exe,
           os.path.join(ROOT, "tests", "hostsim", "refine_vjp_sanitize_main.cpp"), os.path.join(ROOT, "cvxpnpl_amd", "csrc", "host_refine_vjp.cpp")]
    c = subprocess.run(cmd, capture_output=True, text=True)
    if c.returncode != 0 and "sanitize" in c.stderr and "cannot find" in c.stderr:
        pytest.skip("the sanitizer runtimes do not link here")
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and "ok" in p.stdout, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
