"""The argument contract and the plumbing of the RANSAC family's stage wrappers (ransac.py): what a scene set, an active list, a round's
budget, its poses, the seeds and the state of an adaptive call must look like, the message each violation gets, the output buffers of the
samplers, and the one call into a library of the family.  csrc/ransac_entry.h states the same contract for the C entry points.
"""
import ctypes as _C

import numpy as _np
import torch

from . import _lib
from .api import _ptr


def _chk(t, name, dtype, shape, device):
    """What the C entry points assume of a tensor: a contiguous tensor of this dtype and shape on this device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.device != device:
        raise ValueError(f"{name}: on {t.device}, the scenes are on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    return t


def _chk_scenes(sc):
    """sc: ransac.Scenes."""
    dev = sc.device
    if dev.type != "cuda":
        raise ValueError(f"the scenes are on {dev}: cvxpnpl_amd has no CPU path")
    _chk(sc.x, "scene pts_2d", torch.float64, (sc.total, 2), dev)
    _chk(sc.X, "scene pts_3d", torch.float64, (sc.total, 3), dev)
    _chk(sc.offsets, "offsets", torch.int64, (sc.F + 1,), dev)
    _chk(sc.K, "K", torch.float64, (sc.F, 3, 3) if sc.per_scene_K else (3, 3), dev)


def _chk_pnpl_scenes(sc):
    """sc: ransac.PnplScenes."""
    dev = sc.device
    if dev.type != "cuda":
        raise ValueError(f"the scenes are on {dev}: cvxpnpl_amd has no CPU path")
    _chk(sc.x, "scene pts_2d", torch.float64, (sc.total, 2), dev)
    _chk(sc.X, "scene pts_3d", torch.float64, (sc.total, 3), dev)
    _chk(sc.l2, "scene line_2d", torch.float64, (sc.line_total, 2, 2), dev)
    _chk(sc.l3, "scene line_3d", torch.float64, (sc.line_total, 2, 3), dev)
    _chk(sc.offsets, "offsets", torch.int64, (sc.F + 1,), dev)
    _chk(sc.line_offsets, "line_offsets", torch.int64, (sc.F + 1,), dev)
    _chk(sc.K, "K", torch.float64, (sc.F, 3, 3) if sc.per_scene_K else (3, 3), dev)


def _scene_args(sc):
    """d_pt_offsets, n_pts, d_ln_offsets, n_lines of a point-and-line entry point ..."""
    return _ptr(sc.offsets), sc.total, _ptr(sc.line_offsets), sc.line_total


def _data_args(sc):
    """... and its d_pts_2d, d_pts_3d, d_line_2d, d_line_3d."""
    return _ptr(sc.x), _ptr(sc.X), _ptr(sc.l2), _ptr(sc.l3)


def _call(lib, sc, name, *args):
    """Entry point `name` of libcvxpnpl_amd_<lib>.so on the scenes' device and its current stream; a failure raises with the library's
    message."""
    with torch.cuda.device(sc.device):
        L = getattr(_lib, lib + "_lib")()
        rc = getattr(L, name)(*args, _C.c_void_p(torch.cuda.current_stream(sc.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {getattr(L, f'cvxpnpl_{lib}_last_error')().decode()}")


def _usable_mask(usable):
    um = 0
    for s in usable:
        um |= 1 << int(s)
    return um


# ---- the seeds ----

def _seed_words(seeds):
    return _np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=_np.uint64).view(_np.int64)


def _seeds_dev(sc, seeds, packer="pack_scenes"):
    """The sampling seeds as int64 [F] on the scenes' device: those given here (one host-to-device copy), else those packed with the
    scenes by `packer`."""
    if seeds is None:
        if sc.seeds is None:
            raise ValueError(f"no seeds: give them here or to {packer}")
        sd = sc.seeds
    else:
        if len(seeds) != sc.F:
            raise ValueError(f"{len(seeds)} seeds for {sc.F} scenes")
        sd = torch.as_tensor(_seed_words(seeds)).to(sc.device)
    return _chk(sd, "seeds", torch.int64, (sc.F,), sc.device)


def _resolve_seeds(seed, F):
    """The seed keyword of a batch call as F ints: an int (scene f uses seed + f; None draws one), or a sequence of F ints."""
    if seed is None:
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
    if isinstance(seed, (int, _np.integer)):
        return [int(seed) + f for f in range(F)]
    seeds = [int(s) for s in seed]
    if len(seeds) != F:
        raise ValueError(f"{len(seeds)} seeds for {F} scenes")
    return seeds


# ---- the output buffers of the samplers ----

def _sample_outputs(n, sc, want_idx):
    """(p2 [n,4,2], p3 [n,4,3], K_hyp [n,3,3] or None (shared K), idx [n,4] int32 or None) of a point sampler."""
    dev = sc.device
    p2 = torch.empty((n, 4, 2), dtype=torch.float64, device=dev)
    p3 = torch.empty((n, 4, 3), dtype=torch.float64, device=dev)
    Kh = torch.empty((n, 3, 3), dtype=torch.float64, device=dev) if sc.per_scene_K else None
    idx = torch.empty((n, 4), dtype=torch.int32, device=dev) if want_idx else None
    return p2, p3, Kh, idx


def _cost_outputs(n, dev, want_idx):
    """(Q45 [n,45], B27 [n,27], idx [n,4] int32 or None) of a sampler that assembles its minimal costs."""
    Qt = torch.empty((n, 45), dtype=torch.float64, device=dev)
    Bt = torch.empty((n, 27), dtype=torch.float64, device=dev)
    idx = torch.empty((n, 4), dtype=torch.int32, device=dev) if want_idx else None
    return Qt, Bt, idx


# ---- poses, active lists, budgets, the state of an adaptive call ----

def _poses(sc, R, t, status, count, groups, who, min_one=True, required=False):
    """The hypotheses of `groups` scenes (or active entries): R [groups*H,3,3] and t, status, count of that length; returns H.  who: the
    message of an R that is no such tensor; min_one: H = 0 is one too; required: status and count are checked even when None."""
    if not isinstance(R, torch.Tensor) or R.dim() != 3 or R.shape[0] % groups or (min_one and R.shape[0] < groups):
        raise ValueError(who)
    n = R.shape[0]
    _chk(R, "R", torch.float64, (n, 3, 3), sc.device)
    _chk(t, "t", torch.float64, (n, 3), sc.device)
    if required or status is not None:
        _chk(status, "status", torch.int32, (n,), sc.device)
    if required or count is not None:
        _chk(count, "count", torch.int32, (n,), sc.device)
    return n // groups


def _chk_round(sc, A, R, t, status, count=None):
    """The poses of a round: R [A*n_round,3,3] with n_round >= 1, and t, status, count of that length.  Returns n_round."""
    return _poses(sc, R, t, status, count, A, "R must be [n_active*n_round,3,3] with n_round >= 1") if A >= 1 else 0


def _chk_refit(sc, fit, fit_count, R, t, head):
    """What a refit_update reads and writes per scene: the refit (fit.R, fit.t, fit.status), its count, the running pose and head.
    Returns the device."""
    dev = sc.device
    _chk(fit.R, "fit.R", torch.float64, (sc.F, 3, 3), dev)
    _chk(fit.t, "fit.t", torch.float64, (sc.F, 3), dev)
    _chk(fit.status, "fit.status", torch.int32, (sc.F,), dev)
    _chk(fit_count, "fit_count", torch.int32, (sc.F,), dev)
    _chk(R, "R", torch.float64, (sc.F, 3, 3), dev)
    _chk(t, "t", torch.float64, (sc.F, 3), dev)
    _chk(head, "head", torch.int32, (sc.F, 4), dev)
    return dev


def _chk_active(sc, active, n_active):
    """active: int32 on the scenes' device, one dimension, at least n_active entries (the kernels read the first n_active)."""
    A = int(n_active)
    if A < 0:
        raise ValueError("n_active must not be negative")
    if not isinstance(active, torch.Tensor) or active.dim() != 1 or active.shape[0] < A:
        raise ValueError(f"active must be a tensor of at least n_active = {A} entries")
    _chk(active, "active", torch.int32, (active.shape[0],), sc.device)
    return A


def _chk_budget(hyp0, n_round, cap):
    h0, Hr, cp = int(hyp0), int(n_round), int(cap)
    if h0 < 0 or Hr < 0 or cp < 0 or h0 + Hr > cp:
        raise ValueError(f"a round needs 0 <= hyp0, 0 <= n_round and hyp0 + n_round <= cap, got {h0}, {Hr}, {cp}")
    return h0, Hr, cp


def _chk_state(sc, st):
    """st: ransac.AdaptiveState."""
    dev, i32 = sc.device, torch.int32
    for name, shape, dt in (("active", (sc.F,), i32), ("active_next", (sc.F,), i32), ("done", (sc.F,), i32), ("n_active", (1,), i32),
                            ("head", (sc.F, 4), i32), ("best", (sc.F,), i32), ("hyp_used", (sc.F,), i32), ("R", (sc.F, 3, 3), torch.float64),
                            ("t", (sc.F, 3), torch.float64), ("mask", (sc.total,), torch.uint8)):
        _chk(getattr(st, name), "state." + name, dt, shape, dev)
    if st.active.data_ptr() == st.active_next.data_ptr():
        raise ValueError("state.active and state.active_next are the same buffer")


def _chk_state_msac(sc, st):
    """st: ransac.AdaptiveState with best_gain (adaptive_init_msac): the state, and best_gain [F] float64 beside best."""
    _chk_state(sc, st)
    if getattr(st, "best_gain", None) is None:
        raise ValueError("state.best_gain is missing: the state of an MSAC call comes from adaptive_init_msac")
    _chk(st.best_gain, "state.best_gain", torch.float64, (sc.F,), sc.device)


def _chk_gain(sc, gain, n):
    """The gains of n hypotheses: float64 [n] on the scenes' device."""
    return _chk(gain, "gain", torch.float64, (n,), sc.device)


def _chk_scoring(scoring):
    if scoring not in ("count", "msac"):
        raise ValueError(f"scoring must be 'count' or 'msac', got {scoring!r}")
    return scoring


def _chk_pool_full(pool_full):
    if isinstance(pool_full, bool) or not isinstance(pool_full, (int, _np.integer)) or not 0 <= int(pool_full) <= 0x7FFFFFFF:
        raise ValueError(f"pool_full must be an int >= 0 (and below 2^31), got {pool_full!r}")
    return int(pool_full)
