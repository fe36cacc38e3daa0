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
from ._refine_args import _cp, batch_args, host_args, scene_args
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


def _outputs(n, device, want_cov):
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((n, 3, 3), **f64), torch.empty((n, 3), **f64), torch.empty((n, 2), **f64), torch.empty((n,), **i32), torch.empty((n,), **i32),
            torch.empty((n,), **i32), torch.empty((n, 6, 6), **f64) if want_cov else None)


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
    a = batch_args("refine_pose_batch_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines)
    _require_gpu()
    L = _lib.refine_lib()
    oR, ot, cost, iters, ost, n_live, cov = _outputs(a.B, a.dev, want_cov)
    with torch.cuda.device(a.dev):
        rc = L.cvxpnpl_refine_batch(a.B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(a.st),
                                    a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters),
                                    _ptr(ost), _ptr(n_live), _ptr(cov), C.c_void_p(torch.cuda.current_stream(a.dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_batch failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)


def refine_scenes(sc, R, t, mask_pts=None, mask_lines=None, status=None, admit_mask: int = ADMIT_USABLE, max_iters: int = 30, step_tol: float = 1e-10,
                  want_cov: bool = False, sigma_px: float = 0.0) -> RefineResult:
    """Polish one pose per scene of a packed scene set (``ransac.Scenes`` or ``ransac.PnplScenes``): R [F,3,3], t [F,3]; mask_pts [sum P] /
    mask_lines [sum L] uint8 (optional, non-zero = live: e.g. the consensus masks of the RANSAC layers); status [F] int32 (optional, may be
    ``head[:, 0]`` of the RANSAC read-back).  One workgroup per scene, one launch, no synchronisation.  Returns a RefineResult; the
    statuses are those of ``refine_pose_batch`` (4 also for a non-finite number in a live record)."""
    o = _opts(max_iters, step_tol, sigma_px)
    a = scene_args(sc, R, t, status, mask_pts, mask_lines)
    _require_gpu()
    L = _lib.refine_lib()
    oR, ot, cost, iters, ost, n_live, cov = _outputs(a.F, a.dev, want_cov)
    with torch.cuda.device(a.dev):
        rc = L.cvxpnpl_refine_scenes(a.F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3), _ptr(sc.K),
                                     sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), C.byref(o),
                                     _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(cov),
                                     C.c_void_p(torch.cuda.current_stream(a.dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_scenes failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)


def refine_pose_batch_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, status=None, admit_mask: int = ADMIT_USABLE,
                           mask_pts=None, mask_lines=None, max_iters: int = 30, step_tol: float = 1e-10, want_cov: bool = False,
                           sigma_px: float = 0.0, n_threads: int = 0) -> RefineResult:
    """``refine_pose_batch`` on host threads (``cvxpnpl_refine_batch_host``, the same source as the kernels): numpy arrays in and out."""
    o = _opts(max_iters, step_tol, sigma_px)
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines)
    B = a.B
    oR, ot, cost = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 2))
    iters, ost, n_live = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    cov = np.empty((B, 6, 6)) if want_cov else None
    L = _lib.refine_lib()
    rc = L.cvxpnpl_refine_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(a.R), _cp(a.t),
                                     _cp(a.st), 1, int(admit_mask), _cp(a.mp), _cp(a.ml), C.byref(o), _cp(oR), _cp(ot), _cp(cost), _cp(iters), _cp(ost),
                                     _cp(n_live), _cp(cov), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_batch_host failed ({rc}): {L.cvxpnpl_refine_last_error().decode()}")
    return RefineResult(oR, ot, cost, iters, ost, n_live, cov)
