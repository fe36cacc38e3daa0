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

Not here: gradients (``refine_robust_grad.py``, section 18), a covariance under a robust loss and an automatic
scale per problem (``refine_robust_auto.py``, section 22), a ``polish_loss=`` option inside ``ransac_*_batch``.
"""
import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._refine_args import _cp, batch_args, host_args, scene_args
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE

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
    a = batch_args("refine_pose_batch_robust_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    _require_gpu()
    L = _lib.refine_robust_lib()
    B, dev = a.B, a.dev
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(B, dev)
    rw = torch.empty((B, a.n_p + a.n_l), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(a.st),
                                           a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines),
                                           C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw), _ptr(n_in),
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
    o = _opts(loss, scale_px, max_iters, step_tol)
    a = scene_args(sc, R, t, status, mask_pts, mask_lines, weights=(weights_pts, weights_lines))
    _require_gpu()
    L = _lib.refine_robust_lib()
    F, dev = a.F, a.dev
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(F, dev)
    # (zeros: a record outside every scene's slice is written by no workgroup)
    rw_p = torch.zeros((a.n_pts,), dtype=torch.float64, device=dev)
    rw_l = torch.zeros((a.n_lines,), dtype=torch.float64, device=dev) if a.off_l is not None else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3),
                                            _ptr(sc.K), sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, int(admit_mask), _ptr(mask_pts),
                                            _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost),
                                            _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw_p), _ptr(rw_l), _ptr(n_in),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_robust_scenes failed ({rc}): {L.cvxpnpl_refine_robust_last_error().decode()}")
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, (rw_p, rw_l), n_in)


def refine_pose_batch_robust_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px: float = 1.0,
                                  weights_pts=None, weights_lines=None, status=None, admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None,
                                  max_iters: int = 30, step_tol: float = 1e-10, n_threads: int = 0) -> RobustRefineResult:
    """``refine_pose_batch_robust`` on host threads (``cvxpnpl_refine_robust_batch_host``, the same source as the kernels): numpy arrays in
    and out; the weights are float64 arrays of the exact shape."""
    o = _opts(loss, scale_px, max_iters, step_tol)
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    B = a.B
    oR, ot, cost = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 2))
    iters, ost, n_live, n_in = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    rw = np.empty((B, a.n_p + a.n_l))
    L = _lib.refine_robust_lib()
    rc = L.cvxpnpl_refine_robust_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(a.R), _cp(a.t),
                                            _cp(a.st), 1, int(admit_mask), _cp(a.mp), _cp(a.ml), _cp(a.wp), _cp(a.wl), C.byref(o), _cp(oR), _cp(ot),
                                            _cp(cost), _cp(iters), _cp(ost), _cp(n_live), _cp(rw), _cp(n_in), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_robust_batch_host failed ({rc}): {L.cvxpnpl_refine_robust_last_error().decode()}")
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, rw, n_in)
