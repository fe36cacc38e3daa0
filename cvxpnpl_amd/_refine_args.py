"""The argument contract of the refinement family's Python entry points (refine.py, refine_grad.py, refine_robust.py,
refine_robust_grad.py): what a pose, a correspondence pair, a status column, a mask, a weight and an upstream gradient must look like in
the batch, the scenes and the numpy host forms, and the message each violation gets.  Optional arguments are validated when present;
everything here raises before a GPU is asked for.  csrc/refine_entry.h states the same contract for the C entry points.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch


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


def _chk_opt(t, name, dtype, shape, device):
    """_chk of an optional tensor."""
    if t is not None:
        _chk(t, name, dtype, shape, device)


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


def _chk_admit(admit_mask):
    admit_mask = int(admit_mask)
    if admit_mask < 0 or admit_mask > 0xFFFFFFFF:
        raise ValueError("admit_mask: a 32-bit mask of refine statuses")
    return admit_mask


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


def _chk_some(n_p, n_l):
    if n_p == 0 and n_l == 0:
        raise ValueError("need at least one point or line correspondence")


def _np64(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))


def _cp(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size > 0 else C.c_void_p(0)


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


class BatchArgs(NamedTuple):
    B: int
    dev: object
    n_p: int
    n_l: int
    p2: object
    p3: object
    l2: object
    l3: object
    K: object
    per: int       # 1: a K per problem
    st: object
    stride: int


def batch_args(host_form, R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts=None, weights_lines=None,
               grad_R=None, grad_t=None) -> BatchArgs:
    """The inputs of a batch form, validated: contiguous float64 / uint8 tensors on the poses' GPU.  host_form: the name the "no CPU path"
    message points to."""
    if not isinstance(R, torch.Tensor) or R.dim() != 3:
        raise ValueError("R: expected a torch tensor [B,3,3]")
    B, dev = int(R.shape[0]), R.device
    _chk(R, "R", torch.float64, (B, 3, 3), dev)
    _chk(t, "t", torch.float64, (B, 3), dev)
    _chk_opt(grad_R, "grad_R", torch.float64, (B, 3, 3), dev)
    _chk_opt(grad_t, "grad_t", torch.float64, (B, 3), dev)
    p2, p3, n_p = _pair(pts_2d, pts_3d, "points", (2,), (3,), dev, B)
    l2, l3, n_l = _pair(line_2d, line_3d, "lines", (2, 2), (2, 3), dev, B)
    _chk_some(n_p, n_l)
    if not isinstance(K, torch.Tensor) or tuple(K.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"K must be a tensor [3,3] or [{B},3,3]")
    per = int(K.dim() == 3)
    _chk(K, "K", torch.float64, (B, 3, 3) if per else (3, 3), dev)
    st, stride = _chk_status(status, B, dev)
    _chk_opt(mask_pts, "mask_pts", torch.uint8, (B, n_p), dev)
    _chk_opt(mask_lines, "mask_lines", torch.uint8, (B, n_l), dev)
    _chk_opt(weights_pts, "weights_pts", torch.float64, (B, n_p), dev)
    _chk_opt(weights_lines, "weights_lines", torch.float64, (B, n_l), dev)
    if dev.type != "cuda":
        raise ValueError(f"the poses are on {dev}: cvxpnpl_amd has no CPU path ({host_form} is the host form)")
    return BatchArgs(B, dev, n_p, n_l, p2, p3, l2, l3, K, per, st, stride)


class SceneArgs(NamedTuple):
    F: int
    dev: object
    n_pts: int
    n_lines: int
    off_l: object  # the three line tensors of the scene set, None for scenes without lines
    l2: object
    l3: object
    st: object
    stride: int


def scene_args(sc, R, t, status, mask_pts, mask_lines, weights=None, grad_R=None, grad_t=None) -> SceneArgs:
    """The inputs of a scenes form, validated: sc a ``ransac.Scenes`` or ``ransac.PnplScenes``, one pose per scene, packed masks.  weights:
    None for a form that takes none, else the pair (weights_pts, weights_lines)."""
    from . import ransac as _rn

    lines = isinstance(sc, _rn.PnplScenes)
    if not lines and not isinstance(sc, _rn.Scenes):
        raise ValueError("sc: expected ransac.Scenes or ransac.PnplScenes")
    (_rn._chk_pnpl_scenes if lines else _rn._chk_scenes)(sc)
    F, dev = sc.F, sc.device
    _chk(R, "R", torch.float64, (F, 3, 3), dev)
    _chk(t, "t", torch.float64, (F, 3), dev)
    _chk_opt(grad_R, "grad_R", torch.float64, (F, 3, 3), dev)
    _chk_opt(grad_t, "grad_t", torch.float64, (F, 3), dev)
    st, stride = _chk_status(status, F, dev)
    n_pts, n_lines = sc.total, (sc.line_total if lines else 0)
    w_pts, w_lines = weights if weights is not None else (None, None)
    _chk_opt(mask_pts, "mask_pts", torch.uint8, (n_pts,), dev)
    _chk_opt(w_pts, "weights_pts", torch.float64, (n_pts,), dev)
    if not lines and (mask_lines is not None or w_lines is not None):
        if weights is None:
            raise ValueError("mask_lines given for scenes without lines")
        raise ValueError("mask_lines / weights_lines given for scenes without lines")
    _chk_opt(mask_lines, "mask_lines", torch.uint8, (n_lines,), dev)
    _chk_opt(w_lines, "weights_lines", torch.float64, (n_lines,), dev)
    return SceneArgs(F, dev, n_pts, n_lines, *((sc.line_offsets, sc.l2, sc.l3) if lines else (None, None, None)), st, stride)


class HostArgs(NamedTuple):
    B: int
    n_p: int
    n_l: int
    R: object
    t: object
    p2: object
    p3: object
    l2: object
    l3: object
    K: object
    st: object
    mp: object
    ml: object
    wp: object
    wl: object
    gR: object
    gt: object


def host_args(R, t, pts_2d, line_2d, pts_3d, line_3d, K, status, mask_pts, mask_lines, weights_pts=None, weights_lines=None, grad_R=None,
              grad_t=None) -> HostArgs:
    """The inputs of a numpy host form as contiguous arrays of the C types, shapes checked; the weights are taken as they are (float64
    arrays of the exact shape)."""
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
    _chk_some(n_p, n_l)
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
    return HostArgs(B, n_p, n_l, Rn, tn, p2, p3, l2, l3, Kn, st, mp, ml, wp, wl, gR, gt)


def grad_outputs(want, lead_p, lead_l, alloc, weights=False):
    """The gradient outputs of a VJP form by name: alloc(shape) where the kind has records and the name is wanted, else None.  lead_p /
    lead_l: the leading shape of a point / line array ((B, n_p) in the batch forms, (sum P,) in the scenes forms); weights: the two weight
    gradients of the robust forms too."""
    kinds = (("pts_2d", lead_p, (2,)), ("pts_3d", lead_p, (3,)), ("line_2d", lead_l, (2, 2)), ("line_3d", lead_l, (2, 3)))
    if weights:
        kinds += (("weights_pts", lead_p, ()), ("weights_lines", lead_l, ()))
    return {name: alloc(lead + tail) if lead[-1] and name in want else None for name, lead, tail in kinds}
