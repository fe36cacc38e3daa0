"""Robust refinement at a scale per problem, the scale estimated from the data, with a covariance.

``refine_robust.py`` minimises  sum_k w_k rho(s_k)  at one hand-set ``scale_px`` for every problem of a launch and returns no covariance.
The HIP kernels behind libcvxpnpl_amd_refine_robust_auto.so (include/cvxpnpl_amd_refine_robust_auto.h) add what thousands of frames with
different noise levels in one launch need:

- ``robust_scale_batch`` / ``robust_scale_scenes`` / ``robust_scale_batch_host``: sigma per problem from the exact, unweighted median of
  the live records' s_k at a pose:  sigma = sqrt(median(s) / (2 ln 2)).
- ``refine_pose_batch_robust_auto`` / ``refine_scenes_robust_auto`` / ``refine_pose_batch_robust_auto_host``: the loop of
  ``refine_robust.py`` at ``scale = max(scale_factor * sigma, scale_floor_px)`` per problem (or at the caller's scale per problem, or at one
  float as before), for ``scale_rounds`` rounds of estimate-then-polish, optionally with the covariance of the result.
- ``robust_covariance_batch`` / ``robust_covariance_scenes`` / ``robust_covariance_host``: the sandwich covariance
  m / (m - 6) H^-1 B H^-1 of a robustly refined pose in the public chart (w, tau) of ``refine.py``; cov[3:, 3:] is the covariance of t.

Nothing here synchronises or reads back between launches.  Not here (section 22): gradients through the estimated scale or at a scale
per problem, a weighted median, a ``polish_loss=`` option inside ``ransac_*_batch``, a covariance for poses that are not strict minima.
"""
import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._refine_args import _chk, _cp, batch_args, host_args, scene_args
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE
from .refine_robust import RobustRefineResult, _opts, _outputs

__all__ = ["RobustScale", "RobustAutoResult", "RobustCovariance", "robust_scale_batch", "robust_scale_scenes", "robust_scale_batch_host",
           "refine_pose_batch_robust_auto", "refine_scenes_robust_auto", "refine_pose_batch_robust_auto_host", "robust_covariance_batch",
           "robust_covariance_scenes", "robust_covariance_host", "SCALE_FACTOR_95"]

SCALE_FACTOR_95 = 2.4477468306808166  # sqrt(-2 ln 0.05): 95 % of chi_2 residual magnitudes fall inside this many sigma


class RobustScale(NamedTuple):
    sigma_px: object   # [B] sqrt(med_sq / (2 ln 2)); NaN for status 2-4
    med_sq: object     # [B] numpy.median of the live records' s_k
    sq: object         # batch: [B, n_p + n_l]; scenes: ([sum P], [sum L] or None).  s_k; -1 not live; NaN status 2-4
    n_live: object     # [B] int32
    status: object     # [B] int32: the refinement's entry checks (0, 2, 3, 4)


class RobustAutoResult(NamedTuple):
    R: object          # the fields of RobustRefineResult, of the last round (iters: summed over the rounds)
    t: object
    cost: object
    iters: object
    status: object
    n_live: object
    robust_w: object
    n_inlier: object
    scale_px: object   # [B] the scale every problem was polished at; NaN for status 2-4
    sigma_px: object   # [B] the last estimate, None when the scale was given
    cov: object        # [B,6,6] or None
    cov_status: object  # [B] int32 or None: RobustCovariance.status -- a pose that was refined but is not a strict minimum has 3 and a NaN cov


class RobustCovariance(NamedTuple):
    cov: object        # [B,6,6]; NaN unless status is 0
    status: object     # [B] int32: 0 ok, 2 not differentiated, 3 m <= 6 or not a strict minimum, 4 unusable numbers


def _err(L, what, rc, exc=RuntimeError):
    return exc(f"{what} failed ({rc}): {L.cvxpnpl_refine_robust_auto_last_error().decode()}")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _auto_opts(scale_factor, scale_floor_px, scale_rounds):
    try:
        scale_factor, scale_floor_px = float(scale_factor), float(scale_floor_px)
    except (TypeError, ValueError):
        raise ValueError("scale_factor and scale_floor_px must be finite positive numbers") from None
    for name, v in (("scale_factor", scale_factor), ("scale_floor_px", scale_floor_px)):
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite positive number")
    if isinstance(scale_rounds, bool) or not isinstance(scale_rounds, (int, np.integer)) or not 1 <= int(scale_rounds) <= 4:
        raise ValueError("scale_rounds must be an integer from 1 to 4")
    return scale_factor, scale_floor_px, int(scale_rounds)


def _scale_arg(scale_px, n, dev):
    """scale_px of an auto / covariance call: None (estimate), a float (uniform) or a float64 tensor [n] on the poses' device.  Returns
    (the float for the options, the tensor or None)."""
    if scale_px is None:
        return 1.0, None
    if isinstance(scale_px, torch.Tensor):
        _chk(scale_px, "scale_px", torch.float64, (n,), dev)
        return 1.0, scale_px
    if isinstance(scale_px, np.ndarray):
        raise ValueError("scale_px: expected None, a number or a torch tensor")
    return scale_px, None


def _scale_arg_np(scale_px, n):
    if scale_px is None:
        return 1.0, None
    if isinstance(scale_px, np.ndarray):
        if scale_px.dtype != np.float64 or scale_px.shape != (n,) or not scale_px.flags.c_contiguous:
            raise ValueError(f"scale_px: expected a contiguous float64 array [{n}]")
        return 1.0, scale_px
    if isinstance(scale_px, torch.Tensor):
        raise ValueError("scale_px: expected None, a number or a numpy array")
    return scale_px, None


# ---- 1. the scale ----

def _scale_batch_call(a, R, t, K, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask):
    L = _lib.refine_robust_auto_lib()
    B, dev = a.B, a.dev
    sigma, med = torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.float64, device=dev)
    n_live, st = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    sq = torch.empty((B, a.n_p + a.n_l), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_robust_scale_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(a.st), a.stride,
                                          int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), _ptr(sigma), _ptr(med),
                                          _ptr(n_live), _ptr(st), _ptr(sq), _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_scale_batch", rc)
    return RobustScale(sigma, med, sq, n_live, st)


def robust_scale_batch(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, weights_pts=None, weights_lines=None, status=None,
                       admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None) -> RobustScale:
    """sigma of B problems at their poses (R, t) from the median of s_k over the live records; the tensors, ``status`` / ``admit_mask``,
    the masks and the weights are those of ``refine_pose_batch_robust`` (a weight only decides whether a record is live).  Device tensors
    out, nothing synchronised."""
    a = batch_args("robust_scale_batch_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    _require_gpu()
    return _scale_batch_call(a, R, t, K, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask)


def _scale_scenes_call(a, sc, R, t, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask):
    L = _lib.refine_robust_auto_lib()
    F, dev = a.F, a.dev
    sigma, med = torch.empty((F,), dtype=torch.float64, device=dev), torch.empty((F,), dtype=torch.float64, device=dev)
    n_live, st = torch.empty((F,), dtype=torch.int32, device=dev), torch.empty((F,), dtype=torch.int32, device=dev)
    # (-1: a record outside every scene's slice is written by no workgroup and is not live)
    sq_p = torch.full((a.n_pts,), -1.0, dtype=torch.float64, device=dev)
    sq_l = torch.full((a.n_lines,), -1.0, dtype=torch.float64, device=dev) if a.off_l is not None else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_robust_scale_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3), _ptr(sc.K),
                                           sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines),
                                           _ptr(weights_pts), _ptr(weights_lines), _ptr(sigma), _ptr(med), _ptr(n_live), _ptr(st), _ptr(sq_p), _ptr(sq_l),
                                           _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_scale_scenes", rc)
    return RobustScale(sigma, med, (sq_p, sq_l), n_live, st)


def robust_scale_scenes(sc, R, t, weights_pts=None, weights_lines=None, mask_pts=None, mask_lines=None, status=None,
                        admit_mask: int = ADMIT_USABLE) -> RobustScale:
    """``robust_scale_batch`` for one pose per scene of a packed scene set; sq is the pair ([sum P], [sum L] or None)."""
    a = scene_args(sc, R, t, status, mask_pts, mask_lines, weights=(weights_pts, weights_lines))
    _require_gpu()
    return _scale_scenes_call(a, sc, R, t, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask)


def _scale_host_call(a, R, t, admit_mask, n_threads):
    L = _lib.refine_robust_auto_lib()
    B = a.B
    sigma, med, n_live, st = np.empty(B), np.empty(B), np.empty(B, np.int32), np.empty(B, np.int32)
    sq = np.empty((B, a.n_p + a.n_l))
    rc = L.cvxpnpl_robust_scale_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(R), _cp(t), _cp(a.st), 1,
                                           int(admit_mask), _cp(a.mp), _cp(a.ml), _cp(a.wp), _cp(a.wl), _cp(sigma), _cp(med), _cp(n_live), _cp(st), _cp(sq),
                                           int(n_threads))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_scale_batch_host", rc, ValueError)
    return RobustScale(sigma, med, sq, n_live, st)


def robust_scale_batch_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, weights_pts=None, weights_lines=None, status=None,
                            admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None, n_threads: int = 0) -> RobustScale:
    """``robust_scale_batch`` on host threads (the same source as the kernels): numpy arrays in and out."""
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    return _scale_host_call(a, a.R, a.t, admit_mask, n_threads)


# ---- 2. the loop at a scale per problem ----

def _loop_batch_call(a, o, R, t, K, scale, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask):
    L = _lib.refine_robust_auto_lib()
    B, dev = a.B, a.dev
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(B, dev)
    rw = torch.empty((B, a.n_p + a.n_l), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_pp_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(a.st),
                                              a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), _ptr(scale),
                                              C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(ost), _ptr(n_live), _ptr(rw), _ptr(n_in), _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_refine_robust_pp_batch", rc)
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, rw, n_in)


def _loop_scenes_call(a, o, sc, R, t, scale, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask):
    L = _lib.refine_robust_auto_lib()
    F, dev = a.F, a.dev
    oR, ot, cost, iters, ost, n_live, n_in = _outputs(F, dev)
    rw_p = torch.zeros((a.n_pts,), dtype=torch.float64, device=dev)
    rw_l = torch.zeros((a.n_lines,), dtype=torch.float64, device=dev) if a.off_l is not None else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_pp_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3), _ptr(sc.K),
                                               sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, int(admit_mask), _ptr(mask_pts), _ptr(mask_lines),
                                               _ptr(weights_pts), _ptr(weights_lines), _ptr(scale), C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters),
                                               _ptr(ost), _ptr(n_live), _ptr(rw_p), _ptr(rw_l), _ptr(n_in), _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_refine_robust_pp_scenes", rc)
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, (rw_p, rw_l), n_in)


def _loop_host_call(a, o, R, t, scale, admit_mask, n_threads):
    L = _lib.refine_robust_auto_lib()
    B = a.B
    oR, ot, cost = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 2))
    iters, ost, n_live, n_in = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    rw = np.empty((B, a.n_p + a.n_l))
    rc = L.cvxpnpl_refine_robust_pp_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(R), _cp(t), _cp(a.st),
                                               1, int(admit_mask), _cp(a.mp), _cp(a.ml), _cp(a.wp), _cp(a.wl), _cp(scale), C.byref(o), _cp(oR), _cp(ot), _cp(cost),
                                               _cp(iters), _cp(ost), _cp(n_live), _cp(rw), _cp(n_in), int(n_threads))
    if rc != 0:
        raise _err(L, "cvxpnpl_refine_robust_pp_batch_host", rc, ValueError)
    return RobustRefineResult(oR, ot, cost, iters, ost, n_live, rw, n_in)


# ---- 3. the covariance ----

def _cov_batch_call(a, R, t, K, status, loss, scale_f, scale, mask_pts, mask_lines, weights_pts, weights_lines):
    L = _lib.refine_robust_auto_lib()
    B, dev = a.B, a.dev
    cov, cst = torch.empty((B, 6, 6), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_robust_cov_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(status),
                                        _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), _lib.LOSS_NAMES[loss], scale_f, _ptr(scale),
                                        _ptr(cov), _ptr(cst), _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_cov_batch", rc)
    return RobustCovariance(cov, cst)


def _cov_scenes_call(a, sc, R, t, status, loss, scale_f, scale, mask_pts, mask_lines, weights_pts, weights_lines):
    L = _lib.refine_robust_auto_lib()
    F, dev = a.F, a.dev
    cov, cst = torch.empty((F, 6, 6), dtype=torch.float64, device=dev), torch.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_robust_cov_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3), _ptr(sc.K),
                                         sc.per_scene_K, _ptr(R), _ptr(t), _ptr(status), _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts),
                                         _ptr(weights_lines), _lib.LOSS_NAMES[loss], scale_f, _ptr(scale), _ptr(cov), _ptr(cst), _stream(dev))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_cov_scenes", rc)
    return RobustCovariance(cov, cst)


def _cov_host_call(a, R, t, status, loss, scale_f, scale, n_threads):
    L = _lib.refine_robust_auto_lib()
    B = a.B
    cov, cst = np.empty((B, 6, 6)), np.empty(B, np.int32)
    rc = L.cvxpnpl_robust_cov_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(R), _cp(t), _cp(status),
                                         _cp(a.mp), _cp(a.ml), _cp(a.wp), _cp(a.wl), _lib.LOSS_NAMES[loss], scale_f, _cp(scale), _cp(cov), _cp(cst),
                                         int(n_threads))
    if rc != 0:
        raise _err(L, "cvxpnpl_robust_cov_batch_host", rc, ValueError)
    return RobustCovariance(cov, cst)


def _cov_scale(o, loss):
    return 1.0 if loss == "l2" else float(o.scale_px)


def _status_arg(status, n, dev):
    """the refinement's status of the poses of a covariance call: a contiguous int32 tensor [n] or None"""
    if status is not None:
        _chk(status, "status", torch.int32, (n,), dev)
    return status


def robust_covariance_batch(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px=1.0, weights_pts=None,
                            weights_lines=None, status=None, mask_pts=None, mask_lines=None) -> RobustCovariance:
    """The sandwich covariance m / (m - 6) H^-1 B H^-1 of B robustly refined poses (R, t) -- the minimum of sum_k w_k rho(s_k) at ``loss``
    and ``scale_px`` (a float, or a float64 tensor [B]: a scale per problem) -- in the public chart (w, tau).  status [B] int32
    (optional, contiguous): the refinement's status of each pose; only 0 and 1 are differentiated.  Returns RobustCovariance(cov [B,6,6],
    status [B]) of device tensors; nothing is synchronised."""
    if isinstance(R, torch.Tensor) and R.dim() == 3:
        scale_f, scale = _scale_arg(scale_px, int(R.shape[0]), R.device)
        status = _status_arg(status, int(R.shape[0]), R.device)
    else:
        scale_f, scale = scale_px, None
    o = _opts(loss, scale_f, 0, 0.0)
    a = batch_args("robust_covariance_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, None, mask_pts, mask_lines, weights_pts, weights_lines)
    _require_gpu()
    return _cov_batch_call(a, R, t, K, status, loss, _cov_scale(o, loss), scale, mask_pts, mask_lines, weights_pts, weights_lines)


def robust_covariance_scenes(sc, R, t, loss: str = "huber", scale_px=1.0, weights_pts=None, weights_lines=None, mask_pts=None, mask_lines=None,
                             status=None) -> RobustCovariance:
    """``robust_covariance_batch`` for one pose per scene of a packed scene set; ``scale_px`` a float or a tensor [F]."""
    scale_f, scale = (1.0, scale_px) if isinstance(scale_px, torch.Tensor) else (scale_px, None)
    o = _opts(loss, scale_f, 0, 0.0)
    a = scene_args(sc, R, t, None, mask_pts, mask_lines, weights=(weights_pts, weights_lines))
    if scale is not None:
        _chk(scale, "scale_px", torch.float64, (a.F,), a.dev)
    status = _status_arg(status, a.F, a.dev)
    _require_gpu()
    return _cov_scenes_call(a, sc, R, t, status, loss, _cov_scale(o, loss), scale, mask_pts, mask_lines, weights_pts, weights_lines)


def robust_covariance_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px=1.0, weights_pts=None,
                           weights_lines=None, status=None, mask_pts=None, mask_lines=None, n_threads: int = 0) -> RobustCovariance:
    """``robust_covariance_batch`` on host threads: numpy arrays in and out; ``scale_px`` a float or a float64 array [B]."""
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    scale_f, scale = _scale_arg_np(scale_px, a.B)
    o = _opts(loss, scale_f, 0, 0.0)
    return _cov_host_call(a, a.R, a.t, a.st, loss, _cov_scale(o, loss), scale, n_threads)


# ---- the rounds of estimate-then-polish, written once for torch and numpy ----

class _TorchOps:
    where = staticmethod(torch.where)

    @staticmethod
    def scale_of(sigma, factor, floor):
        return torch.clamp(sigma * factor, min=floor)  # (a NaN stays a NaN)

    @staticmethod
    def full(like, value):
        return torch.full_like(like, value)

    @staticmethod
    def zeros_i32(like):
        return torch.zeros_like(like)


class _NumpyOps:
    where = staticmethod(np.where)

    @staticmethod
    def scale_of(sigma, factor, floor):
        return np.maximum(sigma * factor, floor)  # (a NaN stays a NaN)

    @staticmethod
    def full(like, value):
        return np.full_like(like, value)

    @staticmethod
    def zeros_i32(like):
        return np.zeros_like(like)


def _rounds(xp, R, t, scale_f, scale, auto, estimate, loop, covariance, want_cov):
    """estimate(R, t) -> RobustScale;  loop(R, t, scale array or None) -> RobustRefineResult;  covariance(R, t, status, scale array or
    None) -> RobustCovariance.  scale: the caller's array or None; scale_f: the caller's float (scale is None and auto is None); auto: None or
    (factor, floor, rounds)."""
    sigma = None
    if auto is None:
        res = loop(R, t, scale)
        status, iters = res.status, res.iters
        used = scale if scale is not None else xp.full(res.cost[..., 0], float(scale_f))
    else:
        factor, floor, rounds = auto
        cur_R, cur_t, status, iters = R, t, None, None
        for _ in range(rounds):
            est = estimate(cur_R, cur_t)
            used = xp.scale_of(est.sigma_px, factor, floor)
            res = loop(cur_R, cur_t, used)
            st = xp.where(est.status > 1, est.status, res.status)  # (the estimate and the loop make the same entry checks; the estimate names the cause)
            status = st if status is None else xp.where(status > 1, status, st)
            iters = res.iters if iters is None else iters + res.iters
            cur_R, cur_t, sigma = res.R, res.t, est.sigma_px
    failed = status > 1
    nan = xp.full(res.cost[..., 0], float("nan"))
    out_R = xp.where(failed[..., None, None], R, res.R)  # (a problem that any round gave up on: its input pose bit for bit)
    out_t = xp.where(failed[..., None], t, res.t)
    used = xp.where(failed, nan, used)
    iters = xp.where(failed, xp.zeros_i32(iters), iters)
    cov = RobustCovariance(None, None)
    if want_cov:
        cov = covariance(out_R, out_t, status, used if (auto is not None or scale is not None) else None)
    return RobustAutoResult(out_R, out_t, res.cost, iters, status, res.n_live, res.robust_w, res.n_inlier, used, sigma, cov.cov, cov.status)


def refine_pose_batch_robust_auto(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px=None, weights_pts=None,
                                  weights_lines=None, status=None, admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None, max_iters: int = 30,
                                  step_tol: float = 1e-10, scale_factor: float = SCALE_FACTOR_95, scale_floor_px: float = 1e-3, scale_rounds: int = 1,
                                  covariance: bool = False) -> RobustAutoResult:
    """``refine_pose_batch_robust`` at a scale per problem.  scale_px None: for each of ``scale_rounds`` (1-4) rounds, sigma is estimated at
    the current pose (``robust_scale_batch``; round 1 at the input pose) and the loop runs at max(scale_factor sigma, scale_floor_px); a
    float64 tensor [B]: one round at the caller's scales; a float: one round, ``refine_pose_batch_robust``'s result bit for bit.
    covariance=True adds the sandwich covariance of the result and its status (``robust_covariance_batch``: cov, cov_status).  A problem that any round leaves with
    status 2-4 keeps that status, its input pose bit for bit, and NaN in scale_px and cov; under huber and cauchy a scale element that is
    not finite and > 0 gives status 4.  iters is summed over the rounds; cost is the last round's pair, both at the final scale.  Device
    tensors in and out; no synchronisation and no read-back between the launches."""
    factor, floor, rounds = _auto_opts(scale_factor, scale_floor_px, scale_rounds)
    if isinstance(R, torch.Tensor) and R.dim() == 3:
        scale_f, scale = _scale_arg(scale_px, int(R.shape[0]), R.device)
    else:
        scale_f, scale = (1.0 if scale_px is None or isinstance(scale_px, torch.Tensor) else scale_px), None
    o = _opts(loss, scale_f, max_iters, step_tol)
    a = batch_args("refine_pose_batch_robust_auto_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    _require_gpu()
    admit_mask = int(admit_mask)
    return _rounds(_TorchOps, R, t, _cov_scale(o, loss), scale, (factor, floor, rounds) if scale_px is None else None,
                   lambda r, tt: _scale_batch_call(a, r, tt, K, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask),
                   lambda r, tt, s: _loop_batch_call(a, o, r, tt, K, s, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask),
                   lambda r, tt, st, s: _cov_batch_call(a, r, tt, K, st, loss, _cov_scale(o, loss), s, mask_pts, mask_lines, weights_pts, weights_lines),
                   bool(covariance))


def refine_scenes_robust_auto(sc, R, t, loss: str = "huber", scale_px=None, weights_pts=None, weights_lines=None, mask_pts=None, mask_lines=None, status=None,
                              admit_mask: int = ADMIT_USABLE, max_iters: int = 30, step_tol: float = 1e-10, scale_factor: float = SCALE_FACTOR_95,
                              scale_floor_px: float = 1e-3, scale_rounds: int = 1, covariance: bool = False) -> RobustAutoResult:
    """``refine_pose_batch_robust_auto`` for one pose per scene of a packed scene set (``ransac.Scenes`` / ``ransac.PnplScenes``): a scale
    per scene, estimated (scale_px None), given as a float64 tensor [F], or one float as ``refine_scenes_robust``.  robust_w is the pair
    ([sum P], [sum L] or None)."""
    factor, floor, rounds = _auto_opts(scale_factor, scale_floor_px, scale_rounds)
    scale_f, scale = (1.0, scale_px) if scale_px is None or isinstance(scale_px, torch.Tensor) else (scale_px, None)
    o = _opts(loss, scale_f, max_iters, step_tol)
    a = scene_args(sc, R, t, status, mask_pts, mask_lines, weights=(weights_pts, weights_lines))
    if scale is not None:
        _chk(scale, "scale_px", torch.float64, (a.F,), a.dev)
    _require_gpu()
    admit_mask = int(admit_mask)
    return _rounds(_TorchOps, R, t, _cov_scale(o, loss), scale, (factor, floor, rounds) if scale_px is None else None,
                   lambda r, tt: _scale_scenes_call(a, sc, r, tt, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask),
                   lambda r, tt, s: _loop_scenes_call(a, o, sc, r, tt, s, mask_pts, mask_lines, weights_pts, weights_lines, admit_mask),
                   lambda r, tt, st, s: _cov_scenes_call(a, sc, r, tt, st, loss, _cov_scale(o, loss), s, mask_pts, mask_lines, weights_pts, weights_lines),
                   bool(covariance))


def refine_pose_batch_robust_auto_host(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px=None,
                                       weights_pts=None, weights_lines=None, status=None, admit_mask: int = ADMIT_USABLE, mask_pts=None, mask_lines=None,
                                       max_iters: int = 30, step_tol: float = 1e-10, scale_factor: float = SCALE_FACTOR_95, scale_floor_px: float = 1e-3,
                                       scale_rounds: int = 1, covariance: bool = False, n_threads: int = 0) -> RobustAutoResult:
    """``refine_pose_batch_robust_auto`` on host threads (the same sources as the kernels): numpy arrays in and out; ``scale_px`` None, a
    float, or a contiguous float64 array [B]."""
    factor, floor, rounds = _auto_opts(scale_factor, scale_floor_px, scale_rounds)
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines)
    scale_f, scale = _scale_arg_np(scale_px, a.B)
    o = _opts(loss, scale_f, max_iters, step_tol)
    admit_mask = int(admit_mask)

    def c(x):
        return np.ascontiguousarray(x)

    return _rounds(_NumpyOps, a.R, a.t, _cov_scale(o, loss), scale, (factor, floor, rounds) if scale_px is None else None,
                   lambda r, tt: _scale_host_call(a, c(r), c(tt), admit_mask, n_threads),
                   lambda r, tt, s: _loop_host_call(a, o, c(r), c(tt), s, admit_mask, n_threads),
                   lambda r, tt, st, s: _cov_host_call(a, c(r), c(tt), c(st.astype(np.int32)), loss, _cov_scale(o, loss), s, n_threads),
                   bool(covariance))
