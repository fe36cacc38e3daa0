"""TEST-ONLY device twin of tests/hostsim: probe kernels over the device side of cvxpnpl_amd/csrc/solver_core.h, quad_kernel.h and
wave_kernel.h (see devsim.hip / devsim_newton2.hip).  Not part of the product.

Built on first use with the solver library's flags (cvxpnpl_amd/build.py: compile_cmd) and rebuilt when a dependency is newer.  The
hooks shared with hostsim (pospart, proj_affine, dual_lambda, rounds_to, assemble, polar3, ...) take the same arguments and return the
same things, so a test body can be handed either module; every one of them also has a `_batch` form, one problem per lane.

unit: "c3" (the solver library's unit) or "newton2" (lane_kernel.hip's, CVX_REFINE_NEWTON2).
CVXPNPL_DEVSIM_CSRC: another directory to take the product headers from (a scratch copy with a deliberate defect, to see that
the tests notice); the library built from it is kept apart from the real one."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "cvxpnpl_amd", "csrc")
UNITS = ("c3", "newton2")
_PREFIX = {"c3": "ds_", "newton2": "ds2_"}
_lib = None


def csrc():
    return os.path.abspath(os.environ.get("CVXPNPL_DEVSIM_CSRC") or _CSRC_DEFAULT)


def so_path():
    d = csrc()
    if d == os.path.abspath(_CSRC_DEFAULT):
        return os.path.join(_HERE, "libdevsim.so")
    return os.path.join(_HERE, "libdevsim_%s.so" % hashlib.sha1(os.path.relpath(d, _HERE).encode()).hexdigest()[:10])


def sources():
    return [os.path.join(_HERE, n) for n in ("devsim.hip", "devsim_newton2.hip")]


def deps():
    d = csrc()
    return sources() + [os.path.join(_HERE, "devsim_body.h")] + [os.path.join(d, n) for n in sorted(os.listdir(d)) if n.endswith(".h")]


def unit_cmd(src, obj):
    """One translation unit with the flags of cvxpnpl_amd/build.py: compile_cmd() -- no -ffp-contract: what the product's compile does."""
    from cvxpnpl_amd.build import hipcc

    return [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-mllvm", "-enable-ipra=0",
            "-I", csrc(), "-I", _HERE, "-c", "-o", obj, src]


def build(force=False, out=None):
    from cvxpnpl_amd.build import hipcc

    out = out or so_path()
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in deps()):
        with tempfile.TemporaryDirectory() as tmp:
            objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in sources()]
            procs = [subprocess.Popen(unit_cmd(s, o)) for s, o in zip(sources(), objs)]  # (the two units side by side: ~50 s each)
            rcs = [p.wait() for p in procs]
            if any(rcs):
                raise RuntimeError("devsim: hipcc failed (%s)" % rcs)
            subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _fn(unit, name):
    f = getattr(lib(), _PREFIX[unit] + name)
    f.restype = C.c_int
    return f


def _dev(a, dtype):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _check(rc):
    import torch

    if rc != 0:
        raise RuntimeError("devsim: launch failed (hip error %d)" % rc)
    torch.cuda.synchronize()


def _empty(shape, dtype):
    import torch

    return torch.empty(shape, dtype=dtype, device="cuda")


# ---- scalar maps and rotation parameters (device only)

def scalar(name, x, unit="c3"):
    """name: rcp | rsqrt_ | sqrt_fast (cvx::, either unit) | fast_rcp (cvxw::, the solver library's unit only); x [n] float64 -> y [n]"""
    import torch

    xd = _dev(x, np.float64)
    y = _empty(xd.shape, torch.float64)
    if name == "fast_rcp":
        assert unit == "c3"
        _check(lib().ds_fast_rcp(_ptr(xd), _ptr(y), C.c_int(xd.numel())))
    else:
        _check(_fn(unit, "scalar")(C.c_int(("rcp", "rsqrt_", "sqrt_fast").index(name)), _ptr(xd), _ptr(y), C.c_int(xd.numel())))
    return y.cpu().numpy()


ROTATIONS = ("jacobi_cs", "jacobi_cs_dl", "jacobi_cs_dl_exact", "jacobi_cs_f32", "pair_cs", "pair_cs_f64")


def rotation(name, a, rot, tie=None, unit="c3"):
    """The rotation parameters of one Jacobi step.  jacobi_*: a = (al, be, gam) [n, 3]; pair_*: a = (d, gam) [n, 2] and tie [n].
    Returns [n, 3]: (c, s, t) for jacobi_cs / jacobi_cs_f32 / pair_cs, (c, s, dl) for the others; float32 in, float32 out for the
    single-precision ones."""
    import torch

    f32 = name in ("jacobi_cs_f32", "pair_cs")
    ad = _dev(a, np.float32 if f32 else np.float64)
    n = ad.shape[0]
    rd = _dev(rot, np.int32)
    out = _empty((n, 3), torch.float32 if f32 else torch.float64)
    if name in ("pair_cs", "pair_cs_f64"):
        assert unit == "c3" and ad.shape[1] == 2
        td = _dev(tie, np.int32)
        f = lib().ds_pair_f32 if f32 else lib().ds_pair_f64
        _check(f(_ptr(ad), _ptr(rd), _ptr(td), _ptr(out), C.c_int(n)))
    elif f32:
        assert ad.shape[1] == 3
        _check(_fn(unit, "rot_f32")(_ptr(ad), _ptr(rd), _ptr(out), C.c_int(n)))
    else:
        assert ad.shape[1] == 3
        op = ("jacobi_cs", "jacobi_cs_dl", "jacobi_cs_dl_exact").index(name)
        _check(_fn(unit, "rot_f64")(C.c_int(op), _ptr(ad), _ptr(rd), _ptr(out), C.c_int(n)))
    return out.cpu().numpy()


# ---- the hooks hostsim has: batched forms, then hostsim's own call shapes on top of them

def pospart_batch(W55, mode="f64", unit="c3"):
    """mode: f64 (Eig, exact off) | exact (Eig, exact on) | f32 (EigF); W [n, 55] -> Wp [n, 55], lam [n, 10], sweeps [n]"""
    import torch

    W = _dev(np.asarray(W55, dtype=np.float64).reshape(-1, 55), np.float64)
    n = W.shape[0]
    Wp, lam, sw = _empty((n, 55), torch.float64), _empty((n, 10), torch.float64), _empty((n,), torch.int32)
    _check(_fn(unit, "pospart")(C.c_int(("f64", "exact", "f32").index(mode)), _ptr(W), _ptr(Wp), _ptr(lam), _ptr(sw), C.c_int(n)))
    return Wp.cpu().numpy(), lam.cpu().numpy(), sw.cpu().numpy()


def polar3_batch(M, iters=12, unit="c3"):
    import torch

    Md = _dev(np.asarray(M, dtype=np.float64).reshape(-1, 9), np.float64)
    R = _empty(Md.shape, torch.float64)
    _check(_fn(unit, "polar3")(_ptr(Md), _ptr(R), C.c_int(iters), C.c_int(Md.shape[0])))
    return R.cpu().numpy().reshape(-1, 3, 3)


def near_rotation_batch(M, unit="c3"):
    import torch

    Md = _dev(np.asarray(M, dtype=np.float64).reshape(-1, 9), np.float64)
    R = _empty(Md.shape, torch.float64)
    _check(_fn(unit, "near_rotation")(_ptr(Md), _ptr(R), C.c_int(Md.shape[0])))
    return R.cpu().numpy().reshape(-1, 3, 3)


def inv3_batch(M, unit="c3"):
    import torch

    Md = _dev(np.asarray(M, dtype=np.float64).reshape(-1, 9), np.float64)
    Mi, det = _empty(Md.shape, torch.float64), _empty((Md.shape[0],), torch.float64)
    _check(_fn(unit, "inv3")(_ptr(Md), _ptr(Mi), _ptr(det), C.c_int(Md.shape[0])))
    return Mi.cpu().numpy().reshape(-1, 3, 3), det.cpu().numpy()


def proj_affine_batch(E55, homog, variant=0, unit="c3"):
    E = _dev(np.asarray(E55, dtype=np.float64).reshape(-1, 55), np.float64).clone()
    _check(_fn(unit, "proj_affine")(_ptr(E), C.c_int(int(homog)), C.c_int(int(variant)), C.c_int(E.shape[0])))
    return E.cpu().numpy()


def dual_lambda_batch(R, rhs, symm=False, unit="c3"):
    import torch

    Rd = _dev(np.asarray(R, dtype=np.float64).reshape(-1, 9), np.float64)
    hd = _dev(np.asarray(rhs, dtype=np.float64).reshape(-1, 10), np.float64)
    out = _empty(hd.shape, torch.float64)
    _check(_fn(unit, "dual_lambda")(_ptr(Rd), _ptr(hd), C.c_int(int(symm)), _ptr(out), C.c_int(Rd.shape[0])))
    return out.cpu().numpy()


def rounds_to_batch(v, Rp, tol=0.1, unit="c3"):
    import torch

    vd = _dev(np.asarray(v, dtype=np.float64).reshape(-1, 10), np.float64)
    Rd = _dev(np.asarray(Rp, dtype=np.float64).reshape(-1, 9), np.float64)
    ok, d0 = _empty((vd.shape[0],), torch.int32), _empty((vd.shape[0],), torch.float64)
    _check(_fn(unit, "rounds_to")(_ptr(vd), _ptr(Rd), C.c_double(float(tol)), _ptr(ok), _ptr(d0), C.c_int(vd.shape[0])))
    return ok.cpu().numpy() != 0, d0.cpu().numpy()


def assemble_batch(pts_2d, pts_3d, line_2d, line_3d, K, unit="c3"):
    """problem-major batches as at the C ABI ([n, n_p, 2], ...; K [3, 3] or [n, 3, 3]) -> rc [n], B [n, 3, 9], Q [n, 9, 9]"""
    import torch

    a = [_dev(v, np.float64) if v is not None else None for v in (pts_2d, pts_3d, line_2d, line_3d)]
    Kd = _dev(K, np.float64)
    n = a[1].shape[0] if a[1] is not None else a[3].shape[0]
    n_p = a[1].shape[1] if a[1] is not None else 0
    n_l = a[3].shape[1] if a[3] is not None else 0
    B, Q9, rc = _empty((n, 27), torch.float64), _empty((n, 45), torch.float64), _empty((n,), torch.int32)
    _check(_fn(unit, "assemble")(C.c_int(n_p), _ptr(a[0]), _ptr(a[1]), C.c_int(n_l), _ptr(a[2]), _ptr(a[3]), _ptr(Kd), C.c_int(int(Kd.dim() == 3)),
                                 _ptr(B), _ptr(Q9), _ptr(rc), C.c_int(n)))
    Q = np.zeros((n, 9, 9))
    iu = np.triu_indices(9)
    Q[:, iu[0], iu[1]] = Q9.cpu().numpy()
    Q[:, iu[1], iu[0]] = Q[:, iu[0], iu[1]]
    return rc.cpu().numpy(), B.cpu().numpy().reshape(n, 3, 9), Q


def backend(unit="c3", mode="f64"):
    """hostsim's call shapes (one problem per call) over the device build of `unit`; mode: the eigen-solve pospart runs"""
    return _Backend(unit, mode)


class _Backend:
    def __init__(self, unit, mode):
        self.unit, self.mode = unit, mode
        self.name = "devsim[%s,%s]" % (unit, mode)

    def pospart(self, W55):
        Wp, lam, s = pospart_batch(np.asarray(W55)[None], self.mode, self.unit)
        return Wp[0], lam[0], int(s[0])

    def pospart_batch(self, W55, mode=None):
        return pospart_batch(W55, mode or self.mode, self.unit)

    def proj_affine(self, E55, homog):
        return proj_affine_batch(np.asarray(E55)[None], homog, 0, self.unit)[0]

    def proj_affine_rc(self, E55, homog):
        return proj_affine_batch(np.asarray(E55)[None], homog, 1, self.unit)[0]

    def dual_lambda(self, R, rhs, symm=False):
        return dual_lambda_batch(np.asarray(R)[None], np.asarray(rhs)[None], symm, self.unit)[0]

    def rounds_to(self, v, Rp, tol=0.1):
        ok, d0 = rounds_to_batch(np.asarray(v)[None], np.asarray(Rp)[None], tol, self.unit)
        return bool(ok[0]), float(d0[0])

    def assemble(self, pts_2d, pts_3d, line_2d, line_3d, K):
        a = [np.asarray(v, dtype=np.float64)[None] if v is not None else None for v in (pts_2d, pts_3d, line_2d, line_3d)]
        rc, B, Q = assemble_batch(*a, np.asarray(K, dtype=np.float64), self.unit)
        return int(rc[0]), B[0], Q[0]

    def polar3_batch(self, M, iters=12):
        return polar3_batch(M, iters, self.unit)

    def near_rotation_batch(self, M):
        return near_rotation_batch(M, self.unit)

    def inv3_batch(self, M):
        return inv3_batch(M, self.unit)
