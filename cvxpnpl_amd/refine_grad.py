"""Gradients through the reprojection refinement.

A converged refinement is a strict local minimum of the pixel reprojection cost, so the implicit function theorem gives
dL/d(pts_2d, pts_3d, line_2d, line_3d) from dL/dR, dL/dt through one 6x6 solve per problem with the FULL Hessian of the cost and one pass
over the records; the HIP kernels behind ``cvxpnpl_refine_vjp_batch`` / ``cvxpnpl_refine_vjp_scenes`` compute it in float64
(libcvxpnpl_amd_refine_grad.so, include/cvxpnpl_amd_refine_grad.h).  Nothing of the Levenberg-Marquardt iteration is differentiated.  K
gets no gradient, and the pose the iteration started from gets none from the kernels: a minimiser does not depend on its start.

- ``refine_vjp``: the functional form, B problems of one shape (device tensors in, device tensors out, no synchronisation).
- ``refine_vjp_scenes``: packed scenes (``ransac.Scenes`` / ``ransac.PnplScenes``) with optional masks: what ``refine_scenes`` refined.
- ``refine_vjp_host``: the same mathematics on host threads (numpy in and out), for checking.
- ``refine_pose_batch_diff``: ``refine_pose_batch`` as a ``torch.autograd.Function``; chained after ``pnp_batch_diff`` it keeps the graph
  connected for every problem (``pose_passthrough`` is the rule for the input pose).
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._refine_args import _chk_admit, _cp, batch_args, grad_outputs, host_args, scene_args
from .api import _ptr, _require_gpu
from .refine import ADMIT_USABLE, _opts, refine_pose_batch

__all__ = ["refine_vjp", "refine_vjp_scenes", "refine_vjp_host", "refine_pose_batch_diff", "pose_passthrough", "ADMIT_CONVERGED", "GRAD_NAMES"]

ADMIT_CONVERGED = 1 << _lib.REFINE_CONVERGED
GRAD_NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d")


def _chk_want(want):
    want = tuple(want)
    for w in want:
        if w not in GRAD_NAMES:
            raise ValueError(f"want: {w!r} is not one of {GRAD_NAMES}")
    return want


def refine_vjp(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None,
               admit_mask: int = ADMIT_CONVERGED, mask_pts=None, mask_lines=None, want=GRAD_NAMES, want_info: bool = False):
    """dL/d(correspondences) of B refined poses from dL/dR [B,3,3] and dL/dt [B,3] (either may be None: zero), at the poses R, t with the
    refinement's status (the outputs of ``refine_pose_batch``; status None: every problem; a strided column is taken as it is).  The
    correspondences, K and the masks are those the refinement was given: contiguous float64 / uint8 tensors on one GPU.  admit_mask: bit s
    set = refine status s is differentiated (default: converged only).  Returns a dict with the wanted gradients (the inputs' shapes; None
    where the kind is absent or not wanted), ``vjp_status`` [B] int32 (0 differentiated, 1 skipped, 2 singular -- fewer than 3 live
    records or the pose is not a strict minimum --, 3 a live record behind the camera or not finite; for 1-3 every gradient is zero) and,
    with want_info, ``info`` [B,2]: |g| / sum |J||rho| (the stationarity of the pose handed in) and the smallest Cholesky pivot ratio."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    a = batch_args("refine_vjp_host", R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, grad_R=grad_R, grad_t=grad_t)
    _require_gpu()
    L = _lib.refine_grad_lib()
    B, dev = a.B, a.dev
    f64 = dict(dtype=torch.float64, device=dev)
    out = grad_outputs(want, (B, a.n_p), (B, a.n_l), lambda shape: torch.empty(shape, **f64))
    vst = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty((B, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_vjp_batch(B, a.n_p, _ptr(a.p2), _ptr(a.p3), a.n_l, _ptr(a.l2), _ptr(a.l3), _ptr(K), a.per, _ptr(R), _ptr(t), _ptr(a.st),
                                        a.stride, admit_mask, _ptr(mask_pts), _ptr(mask_lines), _ptr(grad_R), _ptr(grad_t), _ptr(out["pts_2d"]),
                                        _ptr(out["pts_3d"]), _ptr(out["line_2d"]), _ptr(out["line_3d"]), _ptr(vst), _ptr(info),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_vjp_batch failed ({rc}): {L.cvxpnpl_refine_grad_last_error().decode()}")
    out["vjp_status"] = vst
    if want_info:
        out["info"] = info
    return out


def refine_vjp_scenes(sc, R, t, status, grad_R=None, grad_t=None, mask_pts=None, mask_lines=None, admit_mask: int = ADMIT_CONVERGED, want=GRAD_NAMES,
                      want_info: bool = False):
    """``refine_vjp`` for one pose per scene of a packed scene set (``ransac.Scenes`` or ``ransac.PnplScenes``), at the poses and statuses
    ``refine_scenes`` returned: R [F,3,3], t [F,3], status [F] int32 or None, grad_R / grad_t the upstream gradients, mask_pts [sum P] /
    mask_lines [sum L] uint8 as the refinement was given them.  The gradients come in the packed layouts [sum P,2], [sum P,3],
    [sum L,2,2], [sum L,2,3] (records that belong to no scene get zero).  One workgroup per scene, one launch, no synchronisation."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    a = scene_args(sc, R, t, status, mask_pts, mask_lines, grad_R=grad_R, grad_t=grad_t)
    _require_gpu()
    L = _lib.refine_grad_lib()
    F, dev = a.F, a.dev
    f64 = dict(dtype=torch.float64, device=dev)
    # (zeros: a record outside every scene's slice is written by no workgroup)
    out = grad_outputs(want, (a.n_pts,), (a.n_lines,), lambda shape: torch.zeros(shape, **f64))
    vst = torch.empty(F, dtype=torch.int32, device=dev)
    info = torch.empty((F, 2), **f64) if want_info else None
    with torch.cuda.device(dev):
        rc = L.cvxpnpl_refine_vjp_scenes(F, _ptr(sc.offsets), a.n_pts, _ptr(a.off_l), a.n_lines, _ptr(sc.x), _ptr(sc.X), _ptr(a.l2), _ptr(a.l3), _ptr(sc.K),
                                         sc.per_scene_K, _ptr(R), _ptr(t), _ptr(a.st), a.stride, admit_mask, _ptr(mask_pts), _ptr(mask_lines),
                                         _ptr(grad_R), _ptr(grad_t), _ptr(out["pts_2d"]), _ptr(out["pts_3d"]), _ptr(out["line_2d"]), _ptr(out["line_3d"]),
                                         _ptr(vst), _ptr(info), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_refine_vjp_scenes failed ({rc}): {L.cvxpnpl_refine_grad_last_error().decode()}")
    out["vjp_status"] = vst
    if want_info:
        out["info"] = info
    return out


def refine_vjp_host(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None,
                    admit_mask: int = ADMIT_CONVERGED, mask_pts=None, mask_lines=None, want=GRAD_NAMES, n_threads: int = 0):
    """``refine_vjp`` on host threads (``cvxpnpl_refine_vjp_batch_host``, the same source as the kernels): numpy arrays in and out; the
    result always holds ``vjp_status`` and ``info``.  The output arrays are filled with NaN before the call: every element the library
    owes is written by it."""
    want, admit_mask = _chk_want(want), _chk_admit(admit_mask)
    a = host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, grad_R=grad_R, grad_t=grad_t)
    B = a.B
    out = grad_outputs(want, (B, a.n_p), (B, a.n_l), lambda shape: np.full(shape, np.nan))
    out.update(vjp_status=np.full(B, -1, np.int32), info=np.full((B, 2), np.nan))
    L = _lib.refine_grad_lib()
    rc = L.cvxpnpl_refine_vjp_batch_host(B, a.n_p, _cp(a.p2), _cp(a.p3), a.n_l, _cp(a.l2), _cp(a.l3), _cp(a.K), int(a.K.ndim == 3), _cp(a.R), _cp(a.t),
                                         _cp(a.st), 1, admit_mask, _cp(a.mp), _cp(a.ml), _cp(a.gR), _cp(a.gt), _cp(out["pts_2d"]), _cp(out["pts_3d"]),
                                         _cp(out["line_2d"]), _cp(out["line_3d"]), _cp(out["vjp_status"]), _cp(out["info"]), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_refine_vjp_batch_host failed ({rc}): {L.cvxpnpl_refine_grad_last_error().decode()}")
    return out


def pose_passthrough(status, grad_R, grad_t):
    """What the pose handed to the refinement receives from the upstream gradients of its outputs, by refine status [B]: for status 2-4
    the pose passed through bit for bit, the Jacobian is the identity and the upstream gradient goes through unchanged; for status 0 and 1
    the output is (an approximation of) a minimiser, which does not depend on the start: zero -- also for a max_iters pose that is not
    differentiated.  grad_R [B,3,3] / grad_t [B,3] may be None (stay None).  Works on any device."""
    through = status >= _lib.REFINE_SKIPPED
    gR = None if grad_R is None else torch.where(through[:, None, None], grad_R, torch.zeros_like(grad_R))
    gt = None if grad_t is None else torch.where(through[:, None], grad_t, torch.zeros_like(grad_t))
    return gR, gt


class _RefinePose(torch.autograd.Function):
    """(R, t, pts_2d, line_2d, pts_3d, line_3d, K, ...) -> (R, t, status); backward by the implicit-function VJP of the minimum."""

    @staticmethod
    def forward(ctx, R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, admit_mask, refine_kw):
        det = [None if x is None else x.detach() for x in (R, t, pts_2d, line_2d, pts_3d, line_3d, K)]
        res = refine_pose_batch(det[0], det[1], pts_2d=det[2], line_2d=det[3], pts_3d=det[4], line_3d=det[5], K=det[6], status=status, mask_pts=mask_pts,
                                mask_lines=mask_lines, **refine_kw)
        ctx.admit_mask = admit_mask
        ctx.save_for_backward(pts_2d, line_2d, pts_3d, line_3d, K, mask_pts, mask_lines, res.R, res.t, res.status)
        ctx.mark_non_differentiable(res.status)
        return res.R, res.t, res.status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_R, grad_t, _grad_status):
        p2, l2, p3, l3, K, mp, ml, R, t, status = ctx.saved_tensors
        need = ctx.needs_input_grad
        gR = grad_R.contiguous() if grad_R is not None else None
        gt = grad_t.contiguous() if grad_t is not None else None
        pR, pt = pose_passthrough(status, gR, gt) if (need[0] or need[1]) else (None, None)
        outs = [None, None, None, None]
        want = tuple(n for n, w in zip(("pts_2d", "line_2d", "pts_3d", "line_3d"), need[2:6]) if w)
        if want:
            g = refine_vjp(R, t, status, gR, gt, pts_2d=p2, line_2d=l2, pts_3d=p3, line_3d=l3, K=K, admit_mask=ctx.admit_mask, mask_pts=mp,
                           mask_lines=ml, want=want)
            outs = [g[n] if w else None for n, w in zip(("pts_2d", "line_2d", "pts_3d", "line_3d"), need[2:6])]
        return (pR if need[0] else None, pt if need[1] else None, *outs, None, None, None, None, None, None)


def refine_pose_batch_diff(R, t, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None, status=None, status_admit_mask: int = ADMIT_USABLE,
                           mask_pts=None, mask_lines=None, max_iters: int = 30, step_tol: float = 1e-10, admit_mask: int = ADMIT_CONVERGED):
    """``refine_pose_batch`` with gradients: returns (R [B,3,3], t [B,3], status [B]) -- the refined poses and the REFINE status.  The
    forward is ``refine_pose_batch`` on the detached inputs, bit-identical to it; ``status`` / ``status_admit_mask`` are its input status
    column and admit mask (the solver's statuses), the other options are its own.  The backward is ``refine_vjp`` for the correspondence
    inputs that require grad, over the refine statuses in ``admit_mask`` (default: converged only; others get zero).  The input pose
    receives ``pose_passthrough``: the upstream gradient unchanged where the pose passed through (refine status 2-4), zero elsewhere, so
    that ``pnp_batch_diff -> refine_pose_batch_diff -> loss`` is a connected graph for every problem.  K, masks and status get None."""
    admit_mask = _chk_admit(admit_mask)
    _opts(max_iters, step_tol, 0.0)
    kw = dict(admit_mask=int(status_admit_mask), max_iters=max_iters, step_tol=step_tol)
    return _RefinePose.apply(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, admit_mask, kw)
