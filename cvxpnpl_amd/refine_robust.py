"""Reprojection refinement under a robust loss and per-correspondence weights.

``refine.py`` minimises the plain sum of squared pixel residuals over a hard uint8 mask.  The HIP kernels behind
``cvxpnpl_refine_robust_batch`` / ``cvxpnpl_refine_robust_scenes`` (libcvxpnpl_amd_refine_robust.so,
include/cvxpnpl_amd_refine_robust.h) minimise  sum_k w_k rho(s_k)  instead -- s_k the squared residual of correspondence k, rho the
L2, Huber or Cauchy loss at scale ``scale_px``, w_k an optional weight (a matcher's confidence) -- on the same Levenberg-Marquardt
schedule, re-weighted at every pose, the whole loop inside one launch.

- ``refine_pose_batch_robust``: B problems of one shape, device tensors in and out, no synchronisation.
- ``refine_scenes_robust``: packed scenes (``ransac.Scenes`` / ``ransac.PnplScenes``); the documented use is to polish a RANSAC pose over
  ALL records of its scene with no mask: ``refine_scenes_robust(sc, R, t, loss="huber", scale_px=thresh, status=head[:, 0])``.
- ``refine_pose_batch_robust_host``: the same mathematics on host threads (numpy in and out), for checking.

Not here: a covariance under a robust loss, gradients (``refine_robust_grad.py``, section 18), a
``polish_loss=`` option inside ``ransac_*_batch``, an automatic scale (MAD).
"""
import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE, _chk, _chk_status, _cp, _np64, _pair

__all__ = ["RobustRefineResult", "refine_pose_batch_robust", "refine_scenes_robust", "refine_pose_batch_robust_host", "LOSSES"]

LOSSES = tuple(_lib.LOSS_NAMES)


class RobustRefineResult(NamedTuple):
    R: object          # [B,3,3]
    t: object          # [B,3]
    cost: object       # [B,2]  sum_k w_k rho(s_k) before and after
    iters: object      # [B] int32
    status: object     # [B] int32, CVXPNPL_REFINE_*
    n_live: object     # [B] int32
    robust_w: object   # batch: [B, n_p + n_l]; scenes: ([sum P], [sum L] or None).  rho'(s_k) at the returned pose; 0 not live; NaN status 2-4
    n_inlier: object   # [B] int32: live records with s_k <= scale_px^2 (n_live for l2; 0 for status 2-4)


def _opts(loss, scale_px, max_iters, step_tol, lambda0=1e-3):
    if not isinstance(loss, str) or loss not in _lib.LOSS_NAMES:
        raise ValueError(f"loss: expected one of {LOSSES}, got {loss!r}")
    try:
        scale_px = float(scale_px)
    except (TypeError, ValueError):
        raise ValueError("scale_px must be a finite positive number") from None
    if loss != "l2" and not (scale_px > 0.0 and math.isfinite(scale_px)):
        raise ValueError("scale_px must be a finite positive number")
    if loss == "l2":
        scale_px = 1.0  # ignored
    max_iters, step_tol, lambda0 = int(max_iters), float(step_tol), float(lambda0)
    if max_iters < 0:
        raise ValueError("max_iters must not be negative")
    for name, v in (("step_tol", step_tol), ("lambda0", lambda0)):
        if not (v >= 0.0) or v == float("inf"):
            raise ValueError(f"{name} must be a finite non-negative number")
    return _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), max_iters, step_tol, lambda0, _lib.LOSS_NAMES[loss], scale_px)


def _outputs(n, device):
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((n, 3, 3), **f64), torch.empty((n, 3), **f64), torch.empty((n, 2), **f64), torch.empty((n,), **i32), torch.empty((n,), **i32),
            torch.empty((n,), **i32), torch.empty((n,), **i32))


def refine_pose_batch_robust(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px: float = 1.0,
                             weights_pts=None, weights_lines=None, status=None, admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None,
                             max_iters: int = 30, step_tol: float = 1e-10) -> RobustRefineResult:
    """Polish B poses on  sum_k w_k rho(s_k).  The tensors, ``status`` / ``admit_mask`` and the masks are those of ``refine_pose_batch``.
    loss: "l2", "huber" or "cauchy" at scale ``scale_px`` (pixels; the residual at which a record stops counting in full; for a line the
    two end-point distances together).  weights_pts [B,n_p] / weights_lines [B,n_l]: optional float64 weights, contiguous, on the
    poses' device; 0 switches a record off like a mask byte (it is not read), a negative or non-finite weight on a record its mask
    admits gives status 4.  Returns a RobustRefineResult of device tensors; nothing is synchronised.  Statuses and pass-through as
    ``refine_pose_batch``; robust_w [B, n_p + n_l] (points then lines)."""
    o = _opts(loss, scale_px, max_iters, step_tol)
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
    if weights_pts is not None:
        _chk(weights_pts, "weights_pts", torch.float64, (B, n_p), dev)
    if weights_lines is not None:
        _chk(weights_lines, "weights_lines", torch.float64, (B, n_l), dev)
    if dev.type != "cuda":
        raise ValueError(f"the poses are on {dev}: cvxpnpl_amd has no CPU path (refine_pose_batch_robust_host is the host form)")
    _require_gpu()
    L = _lib.refine_robust_lib()
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(B, dev)
    rw = torch.empty((B, n_p + n_l), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_batch(B, n_p, _ptr(p2), _ptr(p3), n_l, _ptr(l2), _ptr(l3), _ptr(K), per, _ptr(R), _ptr(t), _ptr(st), stride,
                                           int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), C.byref(o),
                                           _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw), _ptr(n_in),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_robust_batch failed ({rc}): {L.cvxpnpl_refine_robust_last_error().decode()}")
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, rw, n_in)


def refine_scenes_robust(sc, R, t, loss: str = "huber", scale_px: float = 1.0, weights_pts=None, weights_lines=None, mask_pts=None, mask_lines=None,
                         status=None, admit_mask: int = ADMIT_USABLE, max_iters: int = 30, step_tol: float = 1e-10) -> RobustRefineResult:
    """Polish one pose per scene of a packed scene set (``ransac.Scenes`` or ``ransac.PnplScenes``) on the robust cost: R [F,3,3], t [F,3];
    weights_pts [sum P] / weights_lines [sum L] float64 and mask_pts / mask_lines uint8, all optional; status [F] int32 (optional, may be
    ``head[:, 0]`` of the RANSAC read-back).  The use it is made for: a RANSAC pose polished over ALL records of its scene, no mask,
    ``scale_px`` the RANSAC threshold.  One workgroup per scene, no synchronisation.  robust_w is the pair ([sum P], [sum L] or None)."""
    from . import ransac as _rn

    o = _opts(loss, scale_px, max_iters, step_tol)
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
    if weights_pts is not None:
        _chk(weights_pts, "weights_pts", torch.float64, (sc.total,), dev)
    if (mask_lines is not None or weights_lines is not None) and not lines:
        raise ValueError("mask_lines / weights_lines given for scenes without lines")
    if mask_lines is not None:
        _chk(mask_lines, "mask_lines", torch.uint8, (n_lines,), dev)
    if weights_lines is not None:
        _chk(weights_lines, "weights_lines", torch.float64, (n_lines,), dev)
    _require_gpu()
    L = _lib.refine_robust_lib()
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(F, dev)
    # (zeros: a record outside every scene's slice is written by no workgroup)
    rw_p = torch.zeros((sc.total,), dtype=torch.float64, device=dev)
    rw_l = torch.zeros((n_lines,), dtype=torch.float64, device=dev) if lines else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_scenes(F, _ptr(sc.offsets), sc.total, _ptr(sc.line_offsets) if lines else None, n_lines, _ptr(sc.x), _ptr(sc.X),
                                            _ptr(sc.l2) if lines else None, _ptr(sc.l3) if lines else None, _ptr(sc.K), sc.per_scene_K, _ptr(R), _ptr(t),
                                            _ptr(st), stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines),
                                            C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw_p), _ptr(rw_l),
                                            _ptr(n_in), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_robust_scenes failed ({rc}): {L.cvxpnpl_refine_robust_last_error().decode()}")
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, (rw_p, rw_l), n_in)


def _weights_np(w, name, shape):
    if w is None:
        return None
    if not isinstance(w, np.ndarray) or w.dtype != np.float64:
        raise ValueError(f"{name}: expected a float64 numpy array")
    if w.shape != shape:
        raise ValueError(f"{name}: shape {w.shape}, expected {shape}")
    if not w.flags.c_contiguous:
        raise ValueError(f"{name}: not contiguous")
    return w


def refine_pose_batch_robust_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px: float = 1.0,
                                  weights_pts=None, weights_lines=None, status=None, admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None,
                                  max_iters: int = 30, step_tol: float = 1e-10, n_threads: int = 0) -> RobustRefineResult:
    """``refine_pose_batch_robust`` on host threads (``cvxpnpl_refine_robust_batch_host``, the same source as the kernels): numpy arrays in
    and out; the weights are float64 arrays of the exact shape."""
    o = _opts(loss, scale_px, max_iters, step_tol)
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
    wp = _weights_np(weights_pts, "weights_pts", (B, n_p))
    wl = _weights_np(weights_lines, "weights_lines", (B, n_l))
    oR, ot, cost = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 2))
    iters, ost, n_live, n_in = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    rw = np.empty((B, n_p + n_l))
    L = _lib.refine_robust_lib()
    rc = L.cvxpnpl_refine_robust_batch_host(B, n_p, _cp(p2), _cp(p3), n_l, _cp(l2), _cp(l3), _cp(Kn), int(Kn.ndim == 3), _cp(Rn), _cp(tn), _cp(st), 1,
                                            int(admit_mask), _cp(mp), _cp(ml), _cp(wp), _cp(wl), C.byref(o), _cp(oR), _cp(ot), _cp(cost), _cp(iters),
                                            _cp(ost), _cp(n_live), _cp(rw), _cp(n_in), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_robust_batch_host failed ({rc}): {L.cvxpnpl_refine_robust_last_error().decode()}")
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, rw, n_in)
