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
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE, _chk, _chk_status, _cp, _np64, _pair
from .refine_grad import ADMIT_CONVERGED, _chk_admit, pose_passthrough
from .refine_robust import _opts, _weights_np, refine_pose_batch_robust

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
    if not isinstance(R, torch.Tensor) or R.dim() != 3:
        raise ValueError("R: expected a torch tensor [B,3,3]")
    B, dev = int(R.shape[0]), R.device
    _chk(R, "R", torch.float64, (B, 3, 3), dev)
    _chk(t, "t", torch.float64, (B, 3), dev)
    if grad_R is not None:
        _chk(grad_R, "grad_R", torch.float64, (B, 3, 3), dev)
    if grad_t is not None:
        _chk(grad_t, "grad_t", torch.float64, (B, 3), dev)
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
        raise ValueError(f"the poses are on {dev}: cvxpnpl_amd has no CPU path (refine_vjp_robust_host is the host form)")
    _require_gpu()
    L = _lib.refine_robust_grad_lib()
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"pts_2d": torch.empty((B, n_p, 2), **f64) if n_p and "pts_2d" in want else None,
           "pts_3d": torch.empty((B, n_p, 3), **f64) if n_p and "pts_3d" in want else None,
           "line_2d": torch.empty((B, n_l, 2, 2), **f64) if n_l and "line_2d" in want else None,
           "line_3d": torch.empty((B, n_l, 2, 3), **f64) if n_l and "line_3d" in want else None,
           "weights_pts": torch.empty((B, n_p), **f64) if n_p and "weights_pts" in want else None,
           "weights_lines": torch.empty((B, n_l), **f64) if n_l and "weights_lines" in want else None}
    vst = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty((B, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_vjp_batch(B, n_p, _ptr(p2), _ptr(p3), n_l, _ptr(l2), _ptr(l3), _ptr(K), per, _ptr(R), _ptr(t), _ptr(st), stride,
                                               admit_mask, kind, scale, _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts), _ptr(weights_lines),
                                               _ptr(grad_R), _ptr(grad_t), _ptr(out["pts_2d"]), _ptr(out["pts_3d"]), _ptr(out["line_2d"]),
                                               _ptr(out["line_3d"]), _ptr(out["weights_pts"]), _ptr(out["weights_lines"]), _ptr(vst), _ptr(info),
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
    from . import ransac as _rn

    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    kind, scale = _loss(loss, scale_px)
    lines = isinstance(sc, _rn.PnplScenes)
    if not lines and not isinstance(sc, _rn.Scenes):
        raise ValueError("sc: expected ransac.Scenes or ransac.PnplScenes")
    (_rn._chk_pnpl_scenes if lines else _rn._chk_scenes)(sc)
    F, dev = sc.F, sc.device
    _chk(R, "R", torch.float64, (F, 3, 3), dev)
    _chk(t, "t", torch.float64, (F, 3), dev)
    if grad_R is not None:
        _chk(grad_R, "grad_R", torch.float64, (F, 3, 3), dev)
    if grad_t is not None:
        _chk(grad_t, "grad_t", torch.float64, (F, 3), dev)
    st, stride = _chk_status(status, F, dev)
    n_pts, n_lines = sc.total, (sc.line_total if lines else 0)
    if mask_pts is not None:
        _chk(mask_pts, "mask_pts", torch.uint8, (n_pts,), dev)
    if weights_pts is not None:
        _chk(weights_pts, "weights_pts", torch.float64, (n_pts,), dev)
    if (mask_lines is not None or weights_lines is not None) and not lines:
        raise ValueError("mask_lines / weights_lines given for scenes without lines")
    if mask_lines is not None:
        _chk(mask_lines, "mask_lines", torch.uint8, (n_lines,), dev)
    if weights_lines is not None:
        _chk(weights_lines, "weights_lines", torch.float64, (n_lines,), dev)
    _require_gpu()
    L = _lib.refine_robust_grad_lib()
    f64 = dict(dtype=torch.float64, device=dev)
    # (zeros: a record outside every scene's slice is written by no workgroup)
    out = {"pts_2d": torch.zeros((n_pts, 2), **f64) if n_pts and "pts_2d" in want else None,
           "pts_3d": torch.zeros((n_pts, 3), **f64) if n_pts and "pts_3d" in want else None,
           "line_2d": torch.zeros((n_lines, 2, 2), **f64) if n_lines and "line_2d" in want else None,
           "line_3d": torch.zeros((n_lines, 2, 3), **f64) if n_lines and "line_3d" in want else None,
           "weights_pts": torch.zeros((n_pts,), **f64) if n_pts and "weights_pts" in want else None,
           "weights_lines": torch.zeros((n_lines,), **f64) if n_lines and "weights_lines" in want else None}
    vst = torch.empty(F, dtype=torch.int32, device=dev)
    info = torch.empty((F, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_robust_vjp_scenes(F, _ptr(sc.offsets), n_pts, _ptr(sc.line_offsets) if lines else None, n_lines, _ptr(sc.x), _ptr(sc.X),
                                                _ptr(sc.l2) if lines else None, _ptr(sc.l3) if lines else None, _ptr(sc.K), sc.per_scene_K, _ptr(R),
                                                _ptr(t), _ptr(st), stride, admit_mask, kind, scale, _ptr(mask_pts), _ptr(mask_lines), _ptr(weights_pts),
                                                _ptr(weights_lines), _ptr(grad_R), _ptr(grad_t), _ptr(out["pts_2d"]), _ptr(out["pts_3d"]),
                                                _ptr(out["line_2d"]), _ptr(out["line_3d"]), _ptr(out["weights_pts"]), _ptr(out["weights_lines"]),
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
    Rn = _np64(R)
    if Rn.ndim != 3 or Rn.shape[1:] != (3, 3):
        raise ValueError("R: expected [B,3,3]")
    B = Rn.shape[0]
    tn = _np64(t)
    if tn.shape != (B, 3):
        raise ValueError(f"t: expected [{B},3]")
    gR, gt = _np64(grad_R), _np64(grad_t)
    if gR is not None and gR.shape != (B, 3, 3):
        raise ValueError(f"grad_R: expected [{B},3,3]")
    if gt is not None and gt.shape != (B, 3):
        raise ValueError(f"grad_t: expected [{B},3]")
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
    out = {"pts_2d": np.full((B, n_p, 2), np.nan) if n_p and "pts_2d" in want else None,
           "pts_3d": np.full((B, n_p, 3), np.nan) if n_p and "pts_3d" in want else None,
           "line_2d": np.full((B, n_l, 2, 2), np.nan) if n_l and "line_2d" in want else None,
           "line_3d": np.full((B, n_l, 2, 3), np.nan) if n_l and "line_3d" in want else None,
           "weights_pts": np.full((B, n_p), np.nan) if n_p and "weights_pts" in want else None,
           "weights_lines": np.full((B, n_l), np.nan) if n_l and "weights_lines" in want else None,
           "vjp_status": np.full(B, -1, np.int32), "info": np.full((B, 2), np.nan)}
    L = _lib.refine_robust_grad_lib()
    rc = L.cvxpnpl_refine_robust_vjp_batch_host(B, n_p, _cp(p2), _cp(p3), n_l, _cp(l2), _cp(l3), _cp(Kn), int(Kn.ndim == 3), _cp(Rn), _cp(tn), _cp(st), 1,
                                                admit_mask, kind, scale, _cp(mp), _cp(ml), _cp(wp), _cp(wl), _cp(gR), _cp(gt), _cp(out["pts_2d"]),
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
