"""Reprojection refinement of poses.

The solver, its backward pass and the RANSAC refits minimise the reference's algebraic cost; a pose is judged by its pixel reprojection
error.  The HIP kernels behind ``cvxpnpl_refine_batch`` / ``cvxpnpl_refine_scenes`` (libcvxpnpl_amd_refine.so,
include/cvxpnpl_amd_refine.h) run a few Levenberg-Marquardt iterations on pixel residuals in float64, the whole loop inside one launch,
and report a pose covariance from the same normal equations.

- ``refine_pose_batch``: B problems of one shape (the layouts of ``pnpl_batch``), device tensors in and out, no synchronisation.
- ``refine_scenes``: packed scenes of different sizes (``ransac.Scenes`` / ``ransac.PnplScenes``) with optional uint8 masks.
- ``refine_pose_batch_host``: the same mathematics on host threads (numpy in and out), for checking.
"""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .api import _ptr, _require_gpu

__all__ = ["RefineResult", "refine_pose_batch", "refine_scenes", "refine_pose_batch_host", "ADMIT_USABLE"]

ADMIT_USABLE = 0x5  # CERTIFIED | UNCERTIFIED: what the RANSAC layers call usable


class RefineResult(NamedTuple):
    R: object        # [B,3,3]
    t: object        # [B,3]
    cost: object     # [B,2]  sum of squared pixel residuals before and after
    iters: object    # [B] int32
    status: object   # [B] int32, CVXPNPL_REFINE_*
    n_live: object   # [B] int32
    cov: object      # [B,6,6] or None: sigma^2 (J^T J)^-1 in the chart (w, tau), R' = exp([w]x) R, t' = t + tau


def _opts(max_iters, step_tol, sigma_px, lambda0=1e-3):
    max_iters, step_tol, sigma_px, lambda0 = int(max_iters), float(step_tol), float(sigma_px), float(lambda0)
    if max_iters < 0:
        raise ValueError("max_iters must not be negative")
    for name, v in (("step_tol", step_tol), ("sigma_px", sigma_px), ("lambda0", lambda0)):
        if not (v >= 0.0) or v == float("inf"):
            raise ValueError(f"{name} must be a finite non-negative number")
    return _lib.RefineOpts(C.sizeof(_lib.RefineOpts), max_iters, step_tol, lambda0, sigma_px)


def _chk(t, name, dtype, shape, device):
    """What the C entry points assume of a tensor: a contiguous tensor of this dtype and shape on this device (ransac._chk, ValueError
    throughout)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.device != device:
        raise ValueError(f"{name}: on {t.device}, the poses are on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    return t


def _chk_status(status, n, device):
    """status [n] int32, possibly a column of a wider table (head[:, 0] of the RANSAC read-back): returns (tensor, element stride)."""
    if status is None:
        return None, 0
    if not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.dim() != 1 or status.shape[0] != n:
        raise ValueError(f"status: expected an int32 tensor [{n}]")
    if status.device != device:
        raise ValueError(f"status: on {status.device}, the poses are on {device}")
    stride = int(status.stride(0)) if n > 1 else 1
    if stride < 1:
        raise ValueError("status: a positive stride is needed")
    return status, stride


def _outputs(n, device, want_cov):
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((n, 3, 3), **f64), torch.empty((n, 3), **f64), torch.empty((n, 2), **f64), torch.empty((n,), **i32), torch.empty((n,), **i32),
            torch.empty((n,), **i32), torch.empty((n, 6, 6), **f64) if want_cov else None)


def _pair(a2, a3, name, tail2, tail3, device, batch):
    """One kind of correspondence of the batch form: returns (2D, 3D, n) with n = 0 when the pair is absent."""
    if a2 is None and a3 is None:
        return None, None, 0
    if a2 is None or a3 is None:
        raise ValueError(f"{name}: the 2D and the 3D half go together")
    if not isinstance(a3, torch.Tensor) or a3.dim() != 2 + len(tail3):
        raise ValueError(f"{name}: expected 3D tensors [B,n,{','.join(map(str, tail3))}]")
    n = int(a3.shape[1])
    _chk(a3, f"{name} 3D", torch.float64, (batch, n) + tail3, device)
    _chk(a2, f"{name} 2D", torch.float64, (batch, n) + tail2, device)
    return a2, a3, n


def refine_pose_batch(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, status=None, admit_mask: int = ADMIT_USABLE,
                      mask_pts=None, mask_lines=None, max_iters: int = 30, step_tol: float = 1e-10, want_cov: bool = False,
                      sigma_px: float = 0.0) -> RefineResult:
    """Polish B poses on their pixel reprojection error.  R [B,3,3], t [B,3]; pts_2d [B,n_p,2], pts_3d [B,n_p,3], line_2d [B,n_l,2,2],
    line_3d [B,n_l,2,3] (either pair may be None); K [3,3] or [B,3,3]: contiguous float64 tensors on one GPU.  status [B] int32 (optional;
    a strided column is taken as it is) with admit_mask (bit s: status s is refined; default: the solver's 0 and 2); mask_pts [B,n_p] /
    mask_lines [B,n_l] uint8 (optional, non-zero = live).  Returns a RefineResult of device tensors; nothing is synchronised.
    status: 0 converged, 1 max_iters, 2 skipped, 3 singular, 4 a live record behind the camera or with a non-finite number (NaN / inf in
    its 2D or 3D half); for 2-4 the pose is the input pose bit for bit and cost and cov are NaN.  cov (want_cov): sigma^2 (J^T J)^-1 at the final pose with sigma^2 = cost_after / (2 n_live - 6), or sigma_px^2."""
    o = _opts(max_iters, step_tol, sigma_px)
    if not isinstance(R, torch.Tensor) or R.dim() != 3:
        raise ValueError("R: expected a torch tensor [B,3,3]")
    B, dev = int(R.shape[0]), R.device
    _chk(R, "R", torch.float64, (B, 3, 3), dev)
    _chk(t, "t", torch.float64, (B, 3), dev)
    p2, p3, n_p = _pair(pts_2d, pts_3d, "points", (2,), (3,), dev, B)
    l2, l3, n_l = _pair(line_2d, line_3d, "lines", (2, 2), (2, 3), dev, B)
    if n_p == 0 and n_l == 0:
        raise ValueError("need at least one point or line correspondence")
    if not isinstance(K, torch.Tensor) or tuple(K.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"K must be a tensor [3,3] or [{B},3,3]")
    per = int(K.dim() == 3)
    _chk(K, "K", torch.float64, (B, 3, 3) if per else (3, 3), dev)
    st, stride = _chk_status(status, B, dev)
    if mask_pts is not None:
        _chk(mask_pts, "mask_pts", torch.uint8, (B, n_p), dev)
    if mask_lines is not None:
        _chk(mask_lines, "mask_lines", torch.uint8, (B, n_l), dev)
    if dev.type != "cuda":
        raise ValueError(f"the poses are on {dev}: cvxpnpl_amd has no CPU path (refine_pose_batch_host is the host form)")
    _require_gpu()
    L = _lib.refine_lib()
    oR, ot, cost, iters, ost, n_live, cov = _outputs(B, dev, want_cov)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_batch(B, n_p, _ptr(p2), _ptr(p3), n_l, _ptr(l2), _ptr(l3), _ptr(K), per, _ptr(R), _ptr(t), _ptr(st), stride, int(admit_mask),
                                    _ptr(mask_pts), _ptr(mask_lines), C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live),
                                    _ptr(cov), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_batch failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)


def refine_scenes(sc, R, t, mask_pts=None, mask_lines=None, status=None, admit_mask: int = ADMIT_USABLE, max_iters: int = 30, step_tol: float = 1e-10,
                  want_cov: bool = False, sigma_px: float = 0.0) -> RefineResult:
    """Polish one pose per scene of a packed scene set (``ransac.Scenes`` or ``ransac.PnplScenes``): R [F,3,3], t [F,3]; mask_pts [sum P] /
    mask_lines [sum L] uint8 (optional, non-zero = live: e.g. the consensus masks of the RANSAC layers); status [F] int32 (optional, may be
    ``head[:, 0]`` of the RANSAC read-back).  One workgroup per scene, one launch, no synchronisation.  Returns a RefineResult; the
    statuses are those of ``refine_pose_batch`` (4 also for a non-finite number in a live record)."""
    from . import ransac as _rn

    o = _opts(max_iters, step_tol, sigma_px)
    lines = isinstance(sc, _rn.PnplScenes)
    if not lines and not isinstance(sc, _rn.Scenes):
        raise ValueError("sc: expected ransac.Scenes or ransac.PnplScenes")
    (_rn._chk_pnpl_scenes if lines else _rn._chk_scenes)(sc)
    F, dev = sc.F, sc.device
    _chk(R, "R", torch.float64, (F, 3, 3), dev)
    _chk(t, "t", torch.float64, (F, 3), dev)
    st, stride = _chk_status(status, F, dev)
    n_lines = sc.line_total if lines else 0
    if mask_pts is not None:
        _chk(mask_pts, "mask_pts", torch.uint8, (sc.total,), dev)
    if mask_lines is not None:
        if not lines:
            raise ValueError("mask_lines given for scenes without lines")
        _chk(mask_lines, "mask_lines", torch.uint8, (n_lines,), dev)
    _require_gpu()
    L = _lib.refine_lib()
    oR, ot, cost, iters, ost, n_live, cov = _outputs(F, dev, want_cov)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_scenes(F, _ptr(sc.offsets), sc.total, _ptr(sc.line_offsets) if lines else None, n_lines, _ptr(sc.x), _ptr(sc.X),
                                     _ptr(sc.l2) if lines else None, _ptr(sc.l3) if lines else None, _ptr(sc.K), sc.per_scene_K, _ptr(R), _ptr(t), _ptr(st),
                                     stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters),
                                     _ptr(ost), _ptr(n_live), _ptr(cov), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_scenes failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)


def _np64(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))


def _cp(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size > 0 else C.c_void_p(0)


def refine_pose_batch_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, status=None, admit_mask: int = ADMIT_USABLE,
                           mask_pts=None, mask_lines=None, max_iters: int = 30, step_tol: float = 1e-10, want_cov: bool = False,
                           sigma_px: float = 0.0, n_threads: int = 0) -> RefineResult:
    """``refine_pose_batch`` on host threads (``cvxpnpl_refine_batch_host``, the same source as the kernels): numpy arrays in and out."""
    o = _opts(max_iters, step_tol, sigma_px)
    Rn = _np64(R)
    if Rn.ndim != 3 or Rn.shape[1:] != (3, 3):
        raise ValueError("R: expected [B,3,3]")
    B = Rn.shape[0]
    tn = _np64(t)
    if tn.shape != (B, 3):
        raise ValueError(f"t: expected [{B},3]")
    p2, p3, l2, l3 = _np64(pts_2d), _np64(pts_3d), _np64(line_2d), _np64(line_3d)
    n_p = p3.shape[1] if p3 is not None and p3.ndim == 3 else 0
    n_l = l3.shape[1] if l3 is not None and l3.ndim == 4 else 0
    if n_p == 0 and n_l == 0:
        raise ValueError("need at least one point or line correspondence")
    if n_p and (p3.shape != (B, n_p, 3) or p2 is None or p2.shape != (B, n_p, 2)):
        raise ValueError("points: expected pts_2d [B,n_p,2] and pts_3d [B,n_p,3]")
    if n_l and (l3.shape != (B, n_l, 2, 3) or l2 is None or l2.shape != (B, n_l, 2, 2)):
        raise ValueError("lines: expected line_2d [B,n_l,2,2] and line_3d [B,n_l,2,3]")
    Kn = _np64(K)
    if Kn is None or Kn.shape not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"K must be [3,3] or [{B},3,3]")
    st = np.ascontiguousarray(status, dtype=np.int32) if status is not None else None
    if st is not None and st.shape != (B,):
        raise ValueError(f"status: expected [{B}]")
    mp = np.ascontiguousarray(mask_pts, dtype=np.uint8) if mask_pts is not None and n_p else None
    ml = np.ascontiguousarray(mask_lines, dtype=np.uint8) if mask_lines is not None and n_l else None
    if mp is not None and mp.shape != (B, n_p):
        raise ValueError(f"mask_pts: expected [{B},{n_p}]")
    if ml is not None and ml.shape != (B, n_l):
        raise ValueError(f"mask_lines: expected [{B},{n_l}]")
    oR, ot, cost = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 2))
    iters, ost, n_live = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    cov = np.empty((B, 6, 6)) if want_cov else None
    L = _lib.refine_lib()
    rc = L.cvxpnpl_refine_batch_host(B, n_p, _cp(p2), _cp(p3), n_l, _cp(l2), _cp(l3), _cp(Kn), int(Kn.ndim == 3), _cp(Rn), _cp(tn), _cp(st), 1,
                                     int(admit_mask), _cp(mp), _cp(ml), C.byref(o), _cp(oR), _cp(ot), _cp(cost), _cp(iters), _cp(ost), _cp(n_live),
                                     _cp(cov), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_batch_host failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)
