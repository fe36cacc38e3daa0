"""Gradients through the robust reprojection refinement, the weights' included.

A converged robust refinement is a strict local minimum of  F = 1/2 sum_k w_k rho(s_k)  (``refine_robust.py``), so the implicit function
theorem gives dL/d(pts_2d, pts_3d, line_2d, line_3d, weights_pts, weights_lines) from dL/dR, dL/dt through one 6x6 solve per problem
with the FULL Hessian of F -- the rho'' term that the forward iteration drops included -- and one pass over the records; the HIP kernels
behind ``cvxpnpl_refine_robust_vjp_batch`` / ``cvxpnpl_refine_robust_vjp_scenes`` compute it in float64
(libcvxpnpl_amd_refine_robust_grad.so, include/cvxpnpl_amd_refine_robust_grad.h).  Nothing of the iteration is differentiated.  K,
``scale_px`` and the pose the iteration started from get no gradient.

A zero weight is a mask, as in the forward: the record behind it is not read and its weight's gradient is exactly 0, so a confidence
that reaches exactly 0 stays there (parametrise the weights so that they cannot, e.g. as exp of a logit).

- ``refine_vjp_robust``: the functional form, B problems of one shape (device tensors in, device tensors out, no synchronisation).
- ``refine_vjp_scenes_robust``: packed scenes (``ransac.Scenes`` / ``ransac.PnplScenes``): what ``refine_scenes_robust`` refined.
- ``refine_vjp_robust_host``: the same mathematics on host threads (numpy in and out), for checking.
- ``refine_pose_batch_robust_diff``: ``refine_pose_batch_robust`` as a ``torch.autograd.Function``.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._refine_args import _chk_admit, _cp, batch_args, grad_outputs, host_args, scene_args
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE
from .refine_grad import ADMIT_CONVERGED, pose_passthrough
from .refine_robust import _opts, refine_pose_batch_robust

__all__ = ["refine_vjp_robust", "refine_vjp_scenes_robust", "refine_vjp_robust_host", "refine_pose_batch_robust_diff", "ROBUST_GRAD_NAMES"]

ROBUST_GRAD_NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d", "weights_pts", "weights_lines")


def _chk_want(want):
    want = tuple(want)
    for w in want:
        if w not in ROBUST_GRAD_NAMES:
            raise ValueError(f"want: {w!r} is not one of {ROBUST_GRAD_NAMES}")
    return want


def _loss(loss, scale_px):
    o = _opts(loss, scale_px, 0, 0.0)
    return int(o.loss), float(o.scale_px)


def refine_vjp_robust(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber",
                      scale_px: float = 1.0, weights_pts=None, weights_lines=None, admit_mask: int = ADMIT_CONVERGED, mask_pts=None, mask_lines=None,
                      want=ROBUST_GRAD_NAMES, want_info: bool = False):
    """``refine_vjp`` at the minimum of the robust cost: dL/d(correspondences, weights) of B poses refined by ``refine_pose_batch_robust``
    under ``loss`` / ``scale_px`` with the weights weights_pts [B,n_p] / weights_lines [B,n_l] (None: all 1).  Returns ``refine_vjp``'s
    dict plus ``weights_pts`` [B,n_p] and ``weights_lines`` [B,n_l], wanted by name in ``want`` and computable with the weights absent
    (the derivative at w = 1).  A record with weight 0 is not live: it is not read and all its gradients, its weight's included, are
    exactly 0 -- a confidence that reaches exactly 0 stays there.  ``vjp_status`` 3 also covers a negative or non-finite weight on a
    record its mask admits."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    kind, scale = _loss(loss, scale_px)
    a = batch_args("refine_vjp_robust_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines,
                   grad_R, grad_t)
    _require_gpu()
    L = _lib.refine_robust_grad_lib()
    B, dev = a.B, a.dev
    f64 = dict(dtype=torch.float64, device=dev)
    out = grad_outputs(want, (B, a.n_p), (B, a.n_l), lambda shape: torch.empty(shape, **f64), weights=True)
    vst = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty((B, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_vjp_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t),
                                               _ptr(a.st), a.stride, admit_mask, kind, scale, _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts),
                                               _ptr(weights_lines), _ptr(grad_R), _ptr(grad_t), _ptr(out["pts_2d"]), _ptr(out["pts_3d"]),
                                               _ptr(out["line_2d"]), _ptr(out["line_3d"]), _ptr(out["weights_pts"]), _ptr(out["weights_lines"]),
                                               _ptr(vst), _ptr(info),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_robust_vjp_batch failed ({rc}): {L.cvxpnpl_refine_robust_grad_last_error().decode()}")
    out["vjp_status"] = vst
    if want_info:
        out["info"] = info
    return out


def refine_vjp_scenes_robust(sc, R, t, status, grad_R=None, grad_t=None, loss: str = "huber", scale_px: float = 1.0, weights_pts=None,
                             weights_lines=None, mask_pts=None, mask_lines=None, admit_mask: int = ADMIT_CONVERGED, want=ROBUST_GRAD_NAMES,
                             want_info: bool = False):
    """``refine_vjp_robust`` for one pose per scene of a packed scene set (``ransac.Scenes`` or ``ransac.PnplScenes``), at the poses and
    statuses ``refine_scenes_robust`` returned.  weights_pts [sum P] / weights_lines [sum L] and the masks as the refinement was given
    them.  The gradients come in the packed layouts [sum P,2], [sum P,3], [sum L,2,2], [sum L,2,3] and, for the weights, [sum P], [sum L]
    (records that belong to no scene get zero).  One workgroup per scene, one launch, no synchronisation."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    kind, scale = _loss(loss, scale_px)
    a = scene_args(sc, R, t, status, mask_pts, mask_lines, weights=(weights_pts, weights_lines), grad_R=grad_R, grad_t=grad_t)
    _require_gpu()
    L = _lib.refine_robust_grad_lib()
    F, dev = a.F, a.dev
    f64 = dict(dtype=torch.float64, device=dev)
    # (zeros: a record outside every scene's slice is written by no workgroup)
    out = grad_outputs(want, (a.n_pts,), (a.n_lines,), lambda shape: torch.zeros(shape, **f64), weights=True)
    vst = torch.empty(F, dtype=torch.int32, device=dev)
    info = torch.empty((F, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_vjp_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3),
                                                _ptr(sc.K), sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, admit_mask, kind, scale,
                                                _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines), _ptr(grad_R), _ptr(grad_t),
                                                _ptr(out["pts_2d"]), _ptr(out["pts_3d"]), _ptr(out["line_2d"]), _ptr(out["line_3d"]),
                                                _ptr(out["weights_pts"]), _ptr(out["weights_lines"]),
                                                _ptr(vst), _ptr(info), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_robust_vjp_scenes failed ({rc}): {L.cvxpnpl_refine_robust_grad_last_error().decode()}")
    out["vjp_status"] = vst
    if want_info:
        out["info"] = info
    return out


def refine_vjp_robust_host(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber",
                           scale_px: float = 1.0, weights_pts=None, weights_lines=None, admit_mask: int = ADMIT_CONVERGED, mask_pts=None,
                           mask_lines=None, want=ROBUST_GRAD_NAMES, n_threads: int = 0):
    """``refine_vjp_robust`` on host threads (``cvxpnpl_refine_robust_vjp_batch_host``, the same source as the kernels): numpy arrays in
    and out, the weights float64 arrays of the exact shape; the result always holds ``vjp_status`` and ``info``.  The output arrays are
    filled with NaN before the call: every element the library owes is written by it."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    kind, scale = _loss(loss, scale_px)
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts, weights_lines, grad_R, grad_t)
    B = a.B
    out = grad_outputs(want, (B, a.n_p), (B, a.n_l), lambda shape: np.full(shape, np.nan), weights=True)
    out.update(vjp_status=np.full(B, -1, np.int32), info=np.full((B, 2), np.nan))
    L = _lib.refine_robust_grad_lib()
    rc = L.cvxpnpl_refine_robust_vjp_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(a.R),
                                                _cp(a.t), _cp(a.st), 1, admit_mask, kind, scale, _cp(a.mp), _cp(a.ml), _cp(a.wp), _cp(a.wl), _cp(a.gR),
                                                _cp(a.gt), _cp(out["pts_2d"]),
                                                _cp(out["pts_3d"]), _cp(out["line_2d"]), _cp(out["line_3d"]), _cp(out["weights_pts"]),
                                                _cp(out["weights_lines"]), _cp(out["vjp_status"]), _cp(out["info"]), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_robust_vjp_batch_host failed ({rc}): {L.cvxpnpl_refine_robust_grad_last_error().decode()}")
    return out


_DIFF_INPUTS = ("pts_2d", "line_2d", "pts_3d", "line_3d", "weights_pts", "weights_lines")  # inputs 2-7 of _RobustRefinePose.forward


class _RobustRefinePose(torch.autograd.Function):
    """(R, t, pts_2d, line_2d, pts_3d, line_3d, weights_pts, weights_lines, K, ...) -> (R, t, status); backward by the implicit-function
    VJP of the robust minimum."""

    @staticmethod
    def forward(ctx, R, t, pts_2d, line_2d, pts_3d, line_3d, weights_pts, weights_lines, K, status, mask_pts, mask_lines, admit_mask, loss, scale_px,
                refine_kw):
        det = [None if x is None else x.detach() for x in (R, t, pts_2d, line_2d, pts_3d, line_3d, weights_pts, weights_lines, K)]
        res = refine_pose_batch_robust(det[0], det[1], pts_2d=det[2], line_2d=det[3], pts_3d=det[4], line_3d=det[5], K=det[8], loss=loss,
                                       scale_px=scale_px, weights_pts=det[6], weights_lines=det[7], status=status, mask_pts=mask_pts,
                                       mask_lines=mask_lines, **refine_kw)
        ctx.admit_mask, ctx.loss, ctx.scale_px = admit_mask, loss, scale_px
        ctx.save_for_backward(pts_2d, line_2d, pts_3d, line_3d, weights_pts, weights_lines, K, mask_pts, mask_lines, res.R, res.t, res.status)
        ctx.mark_non_differentiable(res.status)
        return res.R, res.t, res.status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_R, grad_t, _grad_status):
        p2, l2, p3, l3, wp, wl, K, mp, ml, R, t, status = ctx.saved_tensors
        need = ctx.needs_input_grad
        gR = grad_R.contiguous() if grad_R is not None else None
        gt = grad_t.contiguous() if grad_t is not None else None
        pR, pt = pose_passthrough(status, gR, gt) if (need[0] or need[1]) else (None, None)
        outs = [None] * 6
        want = tuple(n for n, w in zip(_DIFF_INPUTS, need[2:8]) if w)
        if want:
            g = refine_vjp_robust(R, t, status, gR, gt, pts_2d=p2, line_2d=l2, pts_3d=p3, line_3d=l3, K=K, loss=ctx.loss, scale_px=ctx.scale_px,
                                  weights_pts=wp, weights_lines=wl, admit_mask=ctx.admit_mask, mask_pts=mp, mask_lines=ml, want=want)
            outs = [g[n] if w else None for n, w in zip(_DIFF_INPUTS, need[2:8])]
        return (pR if need[0] else None, pt if need[1] else None, *outs, None, None, None, None, None, None, None, None)


def refine_pose_batch_robust_diff(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, loss: str = "huber", scale_px: float = 1.0,
                                  weights_pts=None, weights_lines=None, status=None, status_admit_mask: int = ADMIT_USABLE, mask_pts=None,
                                  mask_lines=None, max_iters: int = 30, step_tol: float = 1e-10, admit_mask: int = ADMIT_CONVERGED):
    """``refine_pose_batch_robust`` with gradients: returns (R [B,3,3], t [B,3], status [B]).  The forward is ``refine_pose_batch_robust``
    on the detached inputs, bit-identical to it; ``status`` / ``status_admit_mask`` are its input status column and admit mask.  The
    backward is ``refine_vjp_robust`` for whichever of the four correspondence tensors and the two weight tensors require grad, over the
    refine statuses in ``admit_mask`` (default: converged only; others get zero).  A weight that is exactly 0 gets gradient 0 and stays
    there.  The input pose receives ``pose_passthrough``; K, loss, scale, masks and status get None."""
    admit_mask = _chk_admit(admit_mask)
    _opts(loss, scale_px, max_iters, step_tol)
    kw = dict(admit_mask=int(status_admit_mask), max_iters=max_iters, step_tol=step_tol)
    return _RobustRefinePose.apply(R, t, pts_2d, line_2d, pts_3d, line_3d, weights_pts, weights_lines, K, status, mask_pts, mask_lines, admit_mask, loss,
                                   scale_px, kw)
