"""Gradients through the batched pose solves.

A certified pose is the global minimiser of the reference's algebraic cost over O(3) x R^3, so the implicit function theorem gives
dL/d(pts_2d, pts_3d, line_2d, line_3d) from one 6x6 solve per problem; the HIP kernels behind ``cvxpnpl_pose_vjp_batch``
compute it in float64 (libcvxpnpl_amd_grad.so, include/cvxpnpl_amd_grad.h).  Nothing of the iterative solve is differentiated.  K gets no gradient (None).

- ``pose_vjp``: the functional form (device tensors in, device tensors out).
- ``pose_vjp_host``: the same mathematics on host threads (numpy in and out), for checking.
- ``pnpl_batch_diff`` / ``pnp_batch_diff`` / ``pnl_batch_diff``: the ``*_batch`` solves as a ``torch.autograd.Function``;
  they return ``(R, t, status)``, status not differentiable.  Problems that are not differentiated (``certified_only=True``:
  everything but ``CVXPNPL_CERTIFIED``; otherwise every rank-1 status) get zero gradients.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .api import _as_dev, _call, _ptr, _require_gpu, _stream, pnpl_batch

__all__ = ["pose_vjp", "pose_vjp_host", "pnpl_batch_diff", "pnp_batch_diff", "pnl_batch_diff", "ADMIT_CERTIFIED", "ADMIT_RANK1"]

ADMIT_CERTIFIED = 1 << 0  # CVXPNPL_CERTIFIED
ADMIT_RANK1 = 0x15        # CERTIFIED | UNCERTIFIED | REFLECTION: every rank-1 pose


def _shapes(pts_3d, line_3d):
    n_p = pts_3d.shape[-2] if pts_3d is not None and pts_3d.dim() >= 3 else 0
    n_l = line_3d.shape[-3] if line_3d is not None and line_3d.dim() >= 4 else 0
    if n_p == 0 and n_l == 0:
        raise ValueError("need at least one point or line correspondence ([B,n,3] points / [B,n,2,3] lines)")
    batch = (pts_3d if n_p else line_3d).shape[0]
    return batch, n_p, n_l


def pose_vjp(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None,
             admit_mask: int = ADMIT_CERTIFIED, want=("pts_2d", "pts_3d", "line_2d", "line_3d"), want_info: bool = False):
    """dL/d(correspondences) of B pose solves from dL/dR [B,3,3] and dL/dt [B,3] (either may be None: zero), at the poses R, t with
    status (the outputs of ``pnpl_batch``; status None: every problem).  Inputs in the layouts of ``pnpl_batch``, on the GPU.
    Returns a dict with the wanted gradients (float64, the inputs' shapes; None where the correspondence kind is absent), ``vjp_status``
    [B] int32 (CVXPNPL_VJP_*) and, with want_info, ``info`` [B,2] (lambda_min / lambda_max of H, relative |g|)."""
    _require_gpu()
    L = _lib.grad_lib()
    device = R.device
    p3 = _as_dev(pts_3d, device, (3,)) if pts_3d is not None else None
    l3 = _as_dev(line_3d, device, (2, 3)) if line_3d is not None else None
    batch, n_p, n_l = _shapes(p3, l3)
    p2 = _as_dev(pts_2d, device, (2,)) if n_p else None
    l2 = _as_dev(line_2d, device, (2, 2)) if n_l else None
    Kd = _as_dev(K, device, (3, 3))
    per = int(Kd.dim() == 3)
    Rd, td = _as_dev(R, device, (3, 3)), _as_dev(t, device, (3,))
    st = status.to(device=device, dtype=torch.int32).contiguous() if status is not None else None
    gR = _as_dev(grad_R, device, (3, 3)) if grad_R is not None else None
    gt = _as_dev(grad_t, device, (3,)) if grad_t is not None else None
    f64 = dict(device=device, dtype=torch.float64)
    out = {"pts_2d": torch.empty((batch, n_p, 2), **f64) if n_p and "pts_2d" in want else None,
           "pts_3d": torch.empty((batch, n_p, 3), **f64) if n_p and "pts_3d" in want else None,
           "line_2d": torch.empty((batch, n_l, 2, 2), **f64) if n_l and "line_2d" in want else None,
           "line_3d": torch.empty((batch, n_l, 2, 3), **f64) if n_l and "line_3d" in want else None}
    vst = torch.empty(batch, device=device, dtype=torch.int32)
    info = torch.empty((batch, 2), **f64) if want_info else None
    with torch.cuda.device(device):
        _call(L, "cvxpnpl_pose_vjp_batch", batch, n_p, _ptr(p2), _ptr(p3), n_l, _ptr(l2), _ptr(l3), _ptr(Kd), per, _ptr(Rd), _ptr(td), _ptr(st),
              int(admit_mask), _ptr(gR), _ptr(gt), _ptr(out["pts_2d"]), _ptr(out["pts_3d"]), _ptr(out["line_2d"]), _ptr(out["line_3d"]), _ptr(vst),
              _ptr(info), _stream(device), last_error="cvxpnpl_grad_last_error")
    out["vjp_status"] = vst
    if want_info:
        out["info"] = info
    return out


def _np(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))


def _cp(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size > 0 else C.c_void_p(0)


def pose_vjp_host(R, t, status, grad_R=None, grad_t=None, pts_2d=None, line_2d=None, pts_3d=None, line_3d=None, K=None,
                  admit_mask: int = ADMIT_CERTIFIED, n_threads: int = 0):
    """``pose_vjp`` on host threads (``cvxpnpl_pose_vjp_host``, the same source as the kernels): numpy arrays in and out, every
    gradient present in the result, plus ``vjp_status`` and ``info``."""
    L = _lib.grad_lib()
    p3, l3 = _np(pts_3d), _np(line_3d)
    n_p = p3.shape[-2] if p3 is not None and p3.ndim >= 3 else 0
    n_l = l3.shape[-3] if l3 is not None and l3.ndim >= 4 else 0
    if n_p == 0 and n_l == 0:
        raise ValueError("need at least one point or line correspondence")
    batch = (p3 if n_p else l3).shape[0]
    p2 = _np(pts_2d) if n_p else None
    l2 = _np(line_2d) if n_l else None
    Kn = _np(K)
    per = int(Kn.ndim == 3)
    Rn, tn = _np(R).reshape(batch, 9), _np(t).reshape(batch, 3)
    st = np.ascontiguousarray(status, dtype=np.int32) if status is not None else None
    gR = _np(grad_R) if grad_R is not None else None
    gt = _np(grad_t) if grad_t is not None else None
    out = {"pts_2d": np.zeros((batch, n_p, 2)) if n_p else None, "pts_3d": np.zeros((batch, n_p, 3)) if n_p else None,
           "line_2d": np.zeros((batch, n_l, 2, 2)) if n_l else None, "line_3d": np.zeros((batch, n_l, 2, 3)) if n_l else None,
           "vjp_status": np.zeros(batch, np.int32), "info": np.zeros((batch, 2))}
    rc = L.cvxpnpl_pose_vjp_host(batch, n_p, _cp(p2), _cp(p3), n_l, _cp(l2), _cp(l3), _cp(Kn), per, _cp(Rn), _cp(tn), _cp(st), int(admit_mask),
                                 _cp(gR), _cp(gt), _cp(out["pts_2d"]), _cp(out["pts_3d"]), _cp(out["line_2d"]), _cp(out["line_3d"]),
                                 _cp(out["vjp_status"]), _cp(out["info"]), int(n_threads))
    if rc != 0:
        raise ValueError(f"cvxpnpl_pose_vjp_host: bad arguments ({rc})")
    return out


_NAMES = ("pts_2d", "line_2d", "pts_3d", "line_3d")


class _PoseSolve(torch.autograd.Function):
    """(pts_2d, line_2d, pts_3d, line_3d, K) -> (R, t, status); backward by the implicit-function VJP."""

    @staticmethod
    def forward(ctx, pts_2d, line_2d, pts_3d, line_3d, K, admit_mask, solver_kw):
        res = pnpl_batch(pts_2d, line_2d, pts_3d, line_3d, K, **solver_kw)
        ctx.admit_mask = admit_mask
        ins = (pts_2d, line_2d, pts_3d, line_3d, K)
        ctx.plain = [None if isinstance(x, torch.Tensor) else x for x in ins]  # numpy inputs (never differentiated, needed all the same)
        ctx.save_for_backward(*(x if isinstance(x, torch.Tensor) else None for x in ins), res.R, res.t, res.status)
        ctx.mark_non_differentiable(res.status)
        return res.R, res.t, res.status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_R, grad_t, _grad_status):
        *ins, R, t, status = ctx.saved_tensors
        p2, l2, p3, l3, K = (x if x is not None else y for x, y in zip(ins, ctx.plain))
        need = ctx.needs_input_grad[:4]
        if not any(need):
            return (None,) * 7
        want = tuple(n for n, w in zip(_NAMES, need) if w)
        g = pose_vjp(R, t, status, grad_R, grad_t, pts_2d=p2, line_2d=l2, pts_3d=p3, line_3d=l3, K=K, admit_mask=ctx.admit_mask, want=want)
        outs = []
        for name, x, w in zip(_NAMES, (p2, l2, p3, l3), need):
            outs.append(g[name].reshape(x.shape).to(x.dtype) if w else None)
        return (*outs, None, None, None)


def pnpl_batch_diff(pts_2d, line_2d, pts_3d, line_3d, K, eps: float = 1e-9, max_iters: int = 2500, certified_only: bool = True, device=None,
                    **solver_opts):
    """``pnpl_batch`` with gradients: returns (R [B,3,3], t [B,3], status [B]).  R and t carry a grad_fn when an input requires grad;
    the forward is ``pnpl_batch`` on the detached inputs (results bit-identical to it).  certified_only=True: only certified poses are
    differentiated, False: every rank-1 pose (CVXPNPL_UNCERTIFIED / _REFLECTION too).  Others get zero gradients; K gets None."""
    kw = dict(eps=eps, max_iters=max_iters, device=device, **solver_opts)
    return _PoseSolve.apply(pts_2d, line_2d, pts_3d, line_3d, K, ADMIT_CERTIFIED if certified_only else ADMIT_RANK1, kw)


def pnp_batch_diff(pts_2d, pts_3d, K, eps: float = 1e-9, max_iters: int = 2500, certified_only: bool = True, **kw):
    """``pnp_batch`` with gradients (see ``pnpl_batch_diff``)."""
    return pnpl_batch_diff(pts_2d, None, pts_3d, None, K, eps=eps, max_iters=max_iters, certified_only=certified_only, **kw)


def pnl_batch_diff(line_2d, line_3d, K, eps: float = 1e-9, max_iters: int = 2500, certified_only: bool = True, **kw):
    """``pnl_batch`` with gradients (see ``pnpl_batch_diff``)."""
    return pnpl_batch_diff(None, line_2d, None, line_3d, K, eps=eps, max_iters=max_iters, certified_only=certified_only, **kw)
