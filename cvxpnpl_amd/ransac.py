"""RANSAC on top of the batched solver (BASELINE config 5).

The reference has no RANSAC; this is the natural consumer of tens of thousands of minimal
hypotheses per frame: sample 4-subsets, solve them all in one launch, score every hypothesis by
reprojection inliers over the whole scene, refit the best consensus set (assembled on the device from scene + inlier mask,
solved at the cost seam: no host round trip inside a frame).  Sampling, the solves and the scoring are the HIP path (cvxpnpl_sample_minimal_sets, cvxpnpl_solve_batch,
cvxpnpl_score_hypotheses, cvxpnpl_select_best, cvxpnpl_assemble_subsets, cvxpnpl_solve_cost_batch, cvxpnpl_refit_update): no torch kernel in a frame.
"""
from typing import Optional

import numpy as _np
import torch

from . import _lib
from ._ransac_args import (_call, _chk, _chk_active, _chk_budget, _chk_pnpl_scenes, _chk_pool_full, _chk_round, _chk_scenes, _chk_state,  # noqa: F401
                           _chk_gain, _chk_scoring, _chk_state_msac,
                           _chk_refit, _cost_outputs, _data_args, _poses, _resolve_seeds, _sample_outputs, _scene_args, _seed_words, _seeds_dev, _usable_mask)
from .api import _ptr, _require_gpu
from .api import assemble_subsets, pnp_batch, refit_update, sample_minimal_sets, score_hypotheses, select_best, solve_cost_batch


def reprojection_inliers(R: torch.Tensor, t: torch.Tensor, K: torch.Tensor, pts_3d: torch.Tensor, pts_2d: torch.Tensor,
                         thresh: float = 2.0) -> torch.Tensor:
    """[H, M] bool: correspondence m is an inlier of hypothesis h (reprojection error < thresh px, in front
    of the camera).  R [H,3,3], t [H,3], scene pts_3d [M,3], pts_2d [M,2].  (HIP scoring kernel.)"""
    return score_hypotheses(R, t, K, pts_2d, pts_3d, thresh, want_mask=True)[1].bool()


def ransac_pnp(pts_2d, pts_3d, K, n_hyp: int = 4096, thresh: float = 2.0, max_iters: int = 100, eps: float = 1e-6,
               seed: Optional[int] = 0, refit: bool = True, device=None, refit_rounds: int = 1, **solver_opts):
    """Robust PnP for one scene with outliers.

    pts_2d [M,2], pts_3d [M,3] (numpy or torch), K [3,3].  Returns dict with R [3,3], t [3],
    inliers [M] bool, n_inliers, status of the final solve, n_certified hypotheses.  refit_rounds: refits of the consensus set (each one
    assembly + solve + scoring launch; no host synchronisation inside a frame, whatever the count).
    """
    device = _pick_device(device, pts_3d, pts_2d, K)  # like pnpl_batch: the device of a CUDA input, else the current device
    x = torch.as_tensor(pts_2d, dtype=torch.float64, device=device)
    X = torch.as_tensor(pts_3d, dtype=torch.float64, device=device)
    Kd = torch.as_tensor(K, dtype=torch.float64, device=device)
    M = X.shape[0]
    # n_hyp random 4-subsets without replacement, gathered into the solve's inputs by one kernel (cvxpnpl_sample_minimal_sets; round 3 drew
    # them with torch.rand().topk(4): 0.32 ms of a 3.5 ms frame at 50 000 hypotheses)
    if seed is None:
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
    x4, X4 = sample_minimal_sets(x, X, n_hyp, 4, seed)
    res = pnp_batch(x4, X4, Kd, eps=eps, max_iters=max_iters, **solver_opts)  # (solver_opts: e.g. f32_sweeps_until=0, every sweep in float64)
    score = score_hypotheses(res.R, res.t, Kd, x, X, thresh, status=res.status, usable=(0, 2))
    # From here on everything stays on the device until the one read-back at the end, and (round 6) nothing of it is a torch kernel:
    # cvxpnpl_select_best takes the arg-max (lowest index on a tie), gathers the winner's pose and scores it for its inlier MASK; the refit
    # assembles straight from scene + mask (cvxpnpl_assemble_subsets -- the size of the set never leaves the device), solves at the cost
    # seam, and cvxpnpl_refit_update takes the refitted pose, with its own mask and count, when it is usable and keeps at least the
    # consensus it was fitted to.  (Round 5: ~40 small torch kernels around torch.argmax / torch.where, 0.35 ms of a 2.2 ms frame.)
    R, t, head, mask = select_best(score, res.R, res.t, res.status, Kd, x, X, thresh)
    if refit:
        for _ in range(max(1, int(refit_rounds))):  # refit on the consensus set (a second round re-fits the set the first one found)
            Bt, Qt, cnt = assemble_subsets(x, X, Kd, mask)
            fit = solve_cost_batch(Qt, Bt, eps=1e-9, max_iters=2500, device=device)
            refit_update(fit, cnt, Kd, x, X, thresh, R, t, head, mask)
    h = head.cpu()   # the frame's one synchronisation
    return {"R": R[0], "t": t[0], "inliers": mask[0].bool(), "n_inliers": int(h[1]), "status": int(h[0]), "n_certified": int(h[3]), "n_hyp": n_hyp,
            "best_index": int(h[2])}


# ---- many scenes of different sizes in one launch sequence (include/cvxpnpl_amd_ransac.h) -------------------------
# ransac_pnp above handles one scene per call: ~16 launches and one read-back per frame, which at a realistic budget of a few hundred
# hypotheses is almost pure launch latency.  Here F scenes share every launch: F * n_hyp minimal solves in ONE cvxpnpl_solve_batch, F
# refits in ONE cvxpnpl_solve_cost_batch, and the steps around them in the kernels of libcvxpnpl_amd_ransac.so, which address scene f
# through a device array of offsets into the packed correspondences.


class Scenes:
    """F scenes packed on one device: x [total,2], X [total,3] float64, offsets [F+1] int64 (device), sizes (host tuple), K [3,3] or
    [F,3,3], per_scene_K; seeds: the scenes' sampling seeds as int64 [F] on the device, or None.  Built by pack_scenes."""

    def __init__(self, x, X, offsets, sizes, K, seeds=None):
        self.x, self.X, self.offsets, self.sizes, self.K, self.seeds = x, X, offsets, tuple(sizes), K, seeds
        self.F, self.total, self.per_scene_K, self.device = len(self.sizes), int(sum(self.sizes)), int(K.dim() == 3), x.device


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else _np.shape(a)


def _check_scenes(pts_2d, pts_3d, K, sizes):
    """Host-side validation of a scene set (nothing here needs a GPU): returns the sizes.  ValueError for an empty set, a scene of fewer
    than four correspondences, 2D / 3D lengths that differ, sizes that do not add up, or a K that is neither [3,3] nor [F,3,3]."""
    if sizes is None:
        if not isinstance(pts_2d, (list, tuple)) or not isinstance(pts_3d, (list, tuple)):
            raise ValueError("scenes are a list of [M_f,2] and a list of [M_f,3] arrays, or packed [sum M,2] / [sum M,3] arrays with `sizes`")
        if len(pts_2d) != len(pts_3d):
            raise ValueError(f"{len(pts_2d)} scenes of 2D points for {len(pts_3d)} scenes of 3D points")
        sizes = []
        for f, (a, b) in enumerate(zip(pts_2d, pts_3d)):
            sa, sb = _shape(a), _shape(b)
            if len(sa) != 2 or sa[1] != 2 or len(sb) != 2 or sb[1] != 3:
                raise ValueError(f"scene {f}: expected pts_2d [M,2] and pts_3d [M,3], got {sa} and {sb}")
            if sa[0] != sb[0]:
                raise ValueError(f"scene {f}: {sa[0]} 2D points for {sb[0]} 3D points")
            sizes.append(int(sa[0]))
    else:
        sizes = [int(s) for s in sizes]
        sa, sb = _shape(pts_2d), _shape(pts_3d)
        if len(sa) != 2 or sa[1] != 2 or len(sb) != 2 or sb[1] != 3:
            raise ValueError(f"packed scenes: expected pts_2d [sum M,2] and pts_3d [sum M,3], got {sa} and {sb}")
        if sa[0] != sb[0]:
            raise ValueError(f"packed scenes: {sa[0]} 2D points for {sb[0]} 3D points")
        if sum(sizes) != sa[0]:
            raise ValueError(f"sizes add up to {sum(sizes)}, the packed scenes hold {sa[0]} correspondences")
    if len(sizes) == 0:
        raise ValueError("no scenes")
    for f, m in enumerate(sizes):
        if m < 4:
            raise ValueError(f"scene {f} has {m} correspondences: a minimal set needs 4")
    sk = _shape(K)
    if sk != (3, 3) and sk != (len(sizes), 3, 3):
        raise ValueError(f"K must be [3,3] or [{len(sizes)},3,3], got {sk}")
    return sizes


def _pick_device(device, *arrays):
    if device is None:
        for a in arrays:
            for b in (a if isinstance(a, (list, tuple)) else (a,)):
                if isinstance(b, torch.Tensor) and b.is_cuda:
                    return b.device
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _to_dev(a, device):
    if isinstance(a, (list, tuple)):
        if any(isinstance(b, torch.Tensor) for b in a):
            return torch.cat([torch.as_tensor(b, dtype=torch.float64, device=device) for b in a]).contiguous()
        a = _np.concatenate([_np.asarray(b, dtype=_np.float64) for b in a])
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(_np.ascontiguousarray(a, dtype=_np.float64))
    return a.to(device=device, dtype=torch.float64).contiguous()


def pack_scenes(pts_2d, pts_3d, K, sizes=None, device=None, seeds=None) -> Scenes:
    """Validate (on the host) and pack a scene set on the device.  pts_2d / pts_3d: lists of F arrays [M_f,2] / [M_f,3], or packed
    [sum M,2] / [sum M,3] with `sizes`, a host sequence of F ints.  K [3,3] or [F,3,3].  seeds (optional, F ints): the sampling seeds
    travel with the offsets in one copy."""
    sizes = _check_scenes(pts_2d, pts_3d, K, sizes)
    F = len(sizes)
    if seeds is not None and len(seeds) != F:
        raise ValueError(f"{len(seeds)} seeds for {F} scenes")
    _require_gpu()
    device = _pick_device(device, pts_3d, pts_2d, K)
    meta = _np.zeros(F + 1 + (F if seeds is not None else 0), dtype=_np.int64)  # offsets, then the seeds: one host-to-device copy
    _np.cumsum(sizes, out=meta[1:F + 1])
    if seeds is not None:
        meta[F + 1:] = _seed_words(seeds)
    meta = torch.as_tensor(meta).to(device)
    off, sd = meta[:F + 1], (meta[F + 1:] if seeds is not None else None)
    Kd = K if isinstance(K, torch.Tensor) else torch.as_tensor(_np.ascontiguousarray(K, dtype=_np.float64))
    return Scenes(_to_dev(pts_2d, device), _to_dev(pts_3d, device), off, sizes, _to_dev(Kd, device), sd)


def sample_scenes(sc: Scenes, n_hyp: int, seeds=None, want_idx: bool = False):
    """cvxpnpl_ransac_sample_scenes: n_hyp minimal sets per scene, scene f drawing what sample_minimal_sets(scene f, n_hyp, 4, seeds[f]) draws.
    seeds: a sequence of F ints (None: the seeds packed with the scenes).  Returns (p2 [F*n_hyp,4,2], p3 [F*n_hyp,4,3], K_hyp [F*n_hyp,3,3] or None (shared K)) and, with
    want_idx, idx [F*n_hyp,4] int32 (indices within the scene)."""
    _require_gpu()
    _chk_scenes(sc)
    H = int(n_hyp)
    if H < 0:
        raise ValueError("n_hyp must not be negative")
    # (the words before their number is checked: this sampler has always taken an iterable without a len())
    sd = _seeds_dev(sc, seeds if seeds is None else _seed_words(seeds))
    p2, p3, Kh, idx = _sample_outputs(sc.F * H, sc, want_idx)
    _call("ransac", sc, "cvxpnpl_ransac_sample_scenes", sc.F, H, _ptr(sc.offsets), sc.total, _ptr(sd), _ptr(sc.x), _ptr(sc.X),
          _ptr(sc.K) if sc.per_scene_K else None, _ptr(idx), _ptr(p2), _ptr(p3), _ptr(Kh))
    return (p2, p3, Kh, idx) if want_idx else (p2, p3, Kh)


def score_scenes(sc: Scenes, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_score_scenes: count [F*H] int32, the inliers of hypothesis (f, h) = (R, t)[f*H + h] among scene f's correspondences."""
    _require_gpu()
    _chk_scenes(sc)
    H = _poses(sc, R, t, status, None, sc.F, "R must be [F*H,3,3]", min_one=False)
    count = torch.empty((sc.F * H,), dtype=torch.int32, device=sc.device)
    _call("ransac", sc, "cvxpnpl_ransac_score_scenes", sc.F, H, _ptr(sc.offsets), sc.total, _ptr(R), _ptr(t), _ptr(status), _usable_mask(usable), _ptr(sc.K),
          sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(count))
    return count


def select_scenes(sc: Scenes, count, R, t, status, thresh: float = 2.0):
    """cvxpnpl_ransac_select_scenes: per scene the hypothesis of the highest count (lowest index on a tie).  Returns R [F,3,3], t [F,3],
    head [F,4] int32 = (status, inliers, index within the scene, certified hypotheses), mask [total] uint8.  No synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    H, dev = _poses(sc, R, t, status, count, sc.F, "R must be [F*H,3,3] with H >= 1", required=True), sc.device
    oR = torch.empty((sc.F, 3, 3), dtype=torch.float64, device=dev)
    ot = torch.empty((sc.F, 3), dtype=torch.float64, device=dev)
    head = torch.empty((sc.F, 4), dtype=torch.int32, device=dev)
    mask = torch.empty((sc.total,), dtype=torch.uint8, device=dev)
    _call("ransac", sc, "cvxpnpl_ransac_select_scenes", sc.F, H, _ptr(sc.offsets), sc.total, _ptr(count), _ptr(R), _ptr(t), _ptr(status), _ptr(sc.K),
          sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(oR), _ptr(ot), _ptr(head), _ptr(mask))
    return oR, ot, head, mask


def assemble_consensus(sc: Scenes, mask):
    """cvxpnpl_ransac_assemble_consensus: (B27 [F,27], Q45 [F,45], count [F] int32) of every scene's masked correspondences (mask [total]
    uint8, non-zero = taken); feed solve_cost_batch.  Fewer than three taken: NaN for that scene."""
    _require_gpu()
    _chk_scenes(sc)
    dev = sc.device
    _chk(mask, "mask", torch.uint8, (sc.total,), dev)
    Bt = torch.empty((sc.F, 27), dtype=torch.float64, device=dev)
    Qt = torch.empty((sc.F, 45), dtype=torch.float64, device=dev)
    cnt = torch.empty((sc.F,), dtype=torch.int32, device=dev)
    _call("ransac", sc, "cvxpnpl_ransac_assemble_consensus", sc.F, _ptr(sc.offsets), sc.total, _ptr(sc.x), _ptr(sc.X), _ptr(mask), _ptr(sc.K), sc.per_scene_K,
          _ptr(Bt), _ptr(Qt), _ptr(cnt))
    return Bt, Qt, cnt


def refit_update_scenes(sc: Scenes, fit, fit_count, thresh, R, t, head, mask):
    """cvxpnpl_ransac_refit_update_scenes: per scene, take the refitted pose fit.R[f] / fit.t[f] -- pose, status, mask and count together, in
    place -- when it is usable and keeps at least head[f,1] inliers.  One launch, no synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    dev = _chk_refit(sc, fit, fit_count, R, t, head)
    _chk(mask, "mask", torch.uint8, (sc.total,), dev)
    _call("ransac", sc, "cvxpnpl_ransac_refit_update_scenes", sc.F, _ptr(sc.offsets), sc.total, _ptr(fit.R), _ptr(fit.t), _ptr(fit.status), _ptr(fit_count),
          _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(R), _ptr(t), _ptr(head), _ptr(mask))


# ---- a hypothesis budget per scene, solved in rounds (include/cvxpnpl_amd_ransac_adaptive.h) ----------------------
# ransac_pnp_batch(confidence=...) stops a scene once the standard rule says that, at the inlier share its best hypothesis shows, enough
# minimal sets have been drawn.  Round r draws round_hyp further hypotheses for the scenes still ACTIVE; their minimal problems are compact
# (entry a of the active list, hypothesis h of the round: problem a * n_round + h), what lasts over the rounds is indexed by the scene.
# The kernels are those of libcvxpnpl_amd_ransac_adaptive.so; the stage wrappers below check every tensor as _chk does.


class AdaptiveState:
    """What an adaptive call keeps over its rounds, on the scenes' device: active, active_next [F] int32 (the first n entries count),
    n_active [1] int32, done [F] int32, R [F,3,3], t [F,3], head [F,4] int32, best [F] int32 (the count of the running winner), mask
    [total] uint8, hyp_used [F] int32.  Built by adaptive_init.  best_gain: None, or -- an MSAC call, adaptive_init_msac -- [F] float64, the
    gain of the running winner.  lo_taken: None, or -- a call with local optimisation, lo_init -- [F] int32, the refits taken per scene."""

    def __init__(self, F, total, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        self.active, self.active_next, self.done = torch.empty((F,), **i32), torch.empty((F,), **i32), torch.empty((F,), **i32)
        self.n_active, self.head, self.best, self.hyp_used = torch.empty((1,), **i32), torch.empty((F, 4), **i32), torch.empty((F,), **i32), torch.empty((F,), **i32)
        self.R = torch.empty((F, 3, 3), dtype=torch.float64, device=dev)
        self.t = torch.empty((F, 3), dtype=torch.float64, device=dev)
        self.mask = torch.empty((total,), dtype=torch.uint8, device=dev)
        self.best_gain = None
        self.lo_taken = None

    def swap(self):
        """After compact_active: the compacted list becomes the active one."""
        self.active, self.active_next = self.active_next, self.active


def needed_hypotheses(inliers: int, n_corr: int, confidence: float) -> float:
    """cvxpnpl_ransac_adaptive_needed_host: N = log(1 - confidence) / log1p(-q), q = prod_{j<4} (inliers - j) / (n_corr - j), by the function
    the update kernel calls.  inf for inliers < 4, 0 for inliers >= n_corr.  No GPU needed."""
    return float(_lib.ransac_adaptive_lib().cvxpnpl_ransac_adaptive_needed_host(int(inliers), int(n_corr), float(confidence)))


def _check_adaptive(confidence, round_hyp):
    """Host-side validation of the adaptive keywords (nothing here needs a GPU)."""
    c = float(confidence)
    if not (0.0 < c < 1.0):  # (NaN and the infinities compare false)
        raise ValueError(f"confidence must lie inside (0, 1), got {confidence!r}")
    if int(round_hyp) < 1:
        raise ValueError(f"round_hyp must be at least 1, got {round_hyp!r}")
    return c, int(round_hyp)


def adaptive_init(sc: Scenes) -> AdaptiveState:
    """cvxpnpl_ransac_adaptive_init: the state of a call, every scene active, nothing drawn (head[f] = (3, -1, 0, 0), best[f] = -1)."""
    _require_gpu()
    _chk_scenes(sc)
    st = AdaptiveState(sc.F, sc.total, sc.device)
    _call("ransac_adaptive", sc, "cvxpnpl_ransac_adaptive_init", sc.F, _ptr(st.active), _ptr(st.n_active), _ptr(st.head), _ptr(st.best), _ptr(st.hyp_used))
    return st


def sample_active(sc: Scenes, active, n_active: int, hyp0: int, n_round: int, cap: int, seeds=None, want_idx: bool = False):
    """cvxpnpl_ransac_adaptive_sample: for entry a < n_active of `active`, the hypotheses hyp0 .. hyp0 + n_round - 1 of scene active[a] --
    the rows [f, hyp0 : hyp0 + n_round] of sample_scenes(sc, hyp0 + n_round).  Returns (p2 [A*n_round,4,2], p3 [A*n_round,4,3], K_hyp
    [A*n_round,3,3] or None) and, with want_idx, idx [A*n_round,4] int32.  An entry outside [0, F) leaves its rows unwritten."""
    _require_gpu()
    _chk_scenes(sc)
    A = _chk_active(sc, active, n_active)
    h0, Hr, cp = _chk_budget(hyp0, n_round, cap)
    sd = _seeds_dev(sc, seeds)
    p2, p3, Kh, idx = _sample_outputs(A * Hr, sc, want_idx)
    _call("ransac_adaptive", sc, "cvxpnpl_ransac_adaptive_sample", sc.F, A, _ptr(active), h0, Hr, cp, _ptr(sc.offsets), sc.total, _ptr(sd), _ptr(sc.x),
          _ptr(sc.X), _ptr(sc.K) if sc.per_scene_K else None, _ptr(idx), _ptr(p2), _ptr(p3), _ptr(Kh))
    return (p2, p3, Kh, idx) if want_idx else (p2, p3, Kh)


def score_active(sc: Scenes, active, n_active: int, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_adaptive_score: count [A*n_round] int32, the inliers of (R, t)[a*n_round + h] among the correspondences of scene
    active[a]; predicate and status rule of score_scenes."""
    _require_gpu()
    _chk_scenes(sc)
    A = _chk_active(sc, active, n_active)
    Hr = _chk_round(sc, A, R, t, status)
    count = torch.empty((A * Hr,), dtype=torch.int32, device=sc.device)
    _call("ransac_adaptive", sc, "cvxpnpl_ransac_adaptive_score", sc.F, A, _ptr(active), Hr, _ptr(sc.offsets), sc.total, _ptr(R), _ptr(t), _ptr(status),
          _usable_mask(usable), _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(count))
    return count


def update_active(sc: Scenes, st: AdaptiveState, n_active: int, hyp0: int, cap: int, confidence: float, count, R, t, status, thresh: float = 2.0):
    """cvxpnpl_ransac_adaptive_update on the first n_active entries of st.active: the round's best replaces a scene's running best only
    by a strictly higher count (pose, head, best and mask together), certified hypotheses accumulate, hyp_used[f] = hyp0 + n_round, and
    st.done[a] says whether the scene is finished.  n_round is R.shape[0] / n_active.  In place, no synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state(sc, st)
    conf, _ = _check_adaptive(confidence, 1)
    A = _chk_active(sc, st.active, n_active)
    if status is None:
        raise ValueError("status is required")
    Hr = _chk_round(sc, A, R, t, status, count)
    h0, Hr, cp = _chk_budget(hyp0, Hr, cap)
    _call("ransac_adaptive", sc, "cvxpnpl_ransac_adaptive_update", sc.F, A, _ptr(st.active), h0, Hr, cp, conf, _ptr(sc.offsets), sc.total, _ptr(count), _ptr(R),
          _ptr(t), _ptr(status), _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(st.R), _ptr(st.t), _ptr(st.head),
          _ptr(st.best), _ptr(st.mask), _ptr(st.hyp_used), _ptr(st.done))


def compact_active(sc: Scenes, st: AdaptiveState, n_active: int):
    """cvxpnpl_ransac_adaptive_compact: st.active_next = the entries a < n_active of st.active with st.done[a] == 0, in order, and
    st.n_active[0] their number.  No synchronisation; the caller reads st.n_active back and calls st.swap()."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state(sc, st)
    A = _chk_active(sc, st.active, n_active)
    _call("ransac_adaptive", sc, "cvxpnpl_ransac_adaptive_compact", sc.F, A, _ptr(st.active), _ptr(st.done), _ptr(st.active_next), _ptr(st.n_active))


# ---- MSAC scoring: the hypothesis of the lowest truncated quadratic cost (include/cvxpnpl_amd_ransac_msac.h) ------
# ransac_pnp_batch(scoring="msac") selects, per scene, the hypothesis of the highest gain = sum over its inliers of (thresh^2 - r^2) /
# thresh^2 instead of the highest inlier count: where many minimal sets explain all the inliers the count ties and the lowest index
# decides, the gain prefers the pose that fits them best.  The kernels are those of libcvxpnpl_amd_ransac_msac.so, each next to its count
# sibling above; sampling, the solves, the compaction, the refits and the polish are unchanged.


def score_scenes_msac(sc: Scenes, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_msac_score_scenes: (gain [F*H] float64, count [F*H] int32) of hypothesis (f, h) = (R, t)[f*H + h] over scene f.  count is
    score_scenes' count; gain = sum over those inliers of (thresh^2 - r^2) / thresh^2, summed serially in scene order (the same bits from
    score_active_msac and from launch to launch); an unusable hypothesis gains 0.0."""
    _require_gpu()
    _chk_scenes(sc)
    H = _poses(sc, R, t, status, None, sc.F, "R must be [F*H,3,3]", min_one=False)
    gain = torch.empty((sc.F * H,), dtype=torch.float64, device=sc.device)
    count = torch.empty((sc.F * H,), dtype=torch.int32, device=sc.device)
    _call("ransac_msac", sc, "cvxpnpl_ransac_msac_score_scenes", sc.F, H, _ptr(sc.offsets), sc.total, _ptr(R), _ptr(t), _ptr(status), _usable_mask(usable),
          _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(gain), _ptr(count))
    return gain, count


def score_active_msac(sc: Scenes, active, n_active: int, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_msac_score_active: (gain, count) [A*n_round] of (R, t)[a*n_round + h] over scene active[a]; the rows of
    score_scenes_msac bit for bit.  An entry of active outside [0, F) leaves its rows unwritten."""
    _require_gpu()
    _chk_scenes(sc)
    A = _chk_active(sc, active, n_active)
    Hr = _chk_round(sc, A, R, t, status)
    gain = torch.empty((A * Hr,), dtype=torch.float64, device=sc.device)
    count = torch.empty((A * Hr,), dtype=torch.int32, device=sc.device)
    _call("ransac_msac", sc, "cvxpnpl_ransac_msac_score_active", sc.F, A, _ptr(active), Hr, _ptr(sc.offsets), sc.total, _ptr(R), _ptr(t), _ptr(status),
          _usable_mask(usable), _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(gain), _ptr(count))
    return gain, count


def select_scenes_msac(sc: Scenes, gain, R, t, status, thresh: float = 2.0):
    """cvxpnpl_ransac_msac_select_scenes: per scene the hypothesis of the highest gain (lowest index on an exact tie; a gain that is not > 0
    is read as 0).  Returns what select_scenes returns -- R [F,3,3], t [F,3], head [F,4] int32 = (status, inliers, index within the scene,
    certified hypotheses), mask [total] uint8 -- and score [F] float64, the winner's gain.  No synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    H, dev = _poses(sc, R, t, status, None, sc.F, "R must be [F*H,3,3] with H >= 1", required=False), sc.device
    _chk(status, "status", torch.int32, (sc.F * H,), dev)
    _chk_gain(sc, gain, sc.F * H)
    oR = torch.empty((sc.F, 3, 3), dtype=torch.float64, device=dev)
    ot = torch.empty((sc.F, 3), dtype=torch.float64, device=dev)
    head = torch.empty((sc.F, 4), dtype=torch.int32, device=dev)
    mask = torch.empty((sc.total,), dtype=torch.uint8, device=dev)
    score = torch.empty((sc.F,), dtype=torch.float64, device=dev)
    _call("ransac_msac", sc, "cvxpnpl_ransac_msac_select_scenes", sc.F, H, _ptr(sc.offsets), sc.total, _ptr(gain), _ptr(R), _ptr(t), _ptr(status), _ptr(sc.K),
          sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(oR), _ptr(ot), _ptr(head), _ptr(mask), _ptr(score))
    return oR, ot, head, mask, score


def adaptive_init_msac(sc: Scenes) -> AdaptiveState:
    """adaptive_init, then cvxpnpl_ransac_msac_init: the state of an MSAC call, with best_gain [F] float64 = -1 (below every gain)."""
    st = adaptive_init(sc)
    st.best_gain = torch.empty((sc.F,), dtype=torch.float64, device=sc.device)
    _call("ransac_msac", sc, "cvxpnpl_ransac_msac_init", sc.F, _ptr(st.best_gain))
    return st


def update_active_msac(sc: Scenes, st: AdaptiveState, n_active: int, hyp0: int, cap: int, confidence: float, gain, count, R, t, status,
                       thresh: float = 2.0):
    """cvxpnpl_ransac_msac_update on the first n_active entries of st.active: update_active with the gains deciding.  The round's best
    replaces a scene's running best only by a strictly higher gain (pose, head, mask, best -- its count -- and best_gain together); the
    stopping rule reads st.best, the inlier count of the running winner.  In place, no synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state_msac(sc, st)
    conf, _ = _check_adaptive(confidence, 1)
    A = _chk_active(sc, st.active, n_active)
    if status is None:
        raise ValueError("status is required")
    Hr = _chk_round(sc, A, R, t, status, count)
    _chk_gain(sc, gain, A * Hr)
    h0, Hr, cp = _chk_budget(hyp0, Hr, cap)
    _call("ransac_msac", sc, "cvxpnpl_ransac_msac_update", sc.F, A, _ptr(st.active), h0, Hr, cp, conf, _ptr(sc.offsets), sc.total, _ptr(gain), _ptr(count),
          _ptr(R), _ptr(t), _ptr(status), _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(st.R), _ptr(st.t), _ptr(st.head),
          _ptr(st.best), _ptr(st.best_gain), _ptr(st.mask), _ptr(st.hyp_used), _ptr(st.done))


def msac_gain_host(scene_2d, scene_3d, sizes, K, R, t, thresh: float = 2.0, status=None, usable=(0, 2), n_threads: int = 0):
    """cvxpnpl_ransac_msac_score_host: what score_scenes_msac computes, on host arrays by the functions the kernels call.  scene_2d [sum M,2],
    scene_3d [sum M,3] packed with sizes (F ints), K [3,3] or [F,3,3], R [F*H,3,3], t [F*H,3], status [F*H] or None.  Returns numpy
    (gain [F*H] float64, count [F*H] int32).  No GPU needed."""
    import ctypes as C

    szs = [int(m) for m in sizes]
    F, total = len(szs), sum(szs)
    if F < 1 or any(m < 0 for m in szs):
        raise ValueError("sizes: at least one scene, no negative size")
    x = _np.ascontiguousarray(scene_2d, dtype=_np.float64)
    X = _np.ascontiguousarray(scene_3d, dtype=_np.float64)
    Kh = _np.ascontiguousarray(K, dtype=_np.float64)
    Rh = _np.ascontiguousarray(R, dtype=_np.float64)
    th = _np.ascontiguousarray(t, dtype=_np.float64)
    if x.shape != (total, 2) or X.shape != (total, 3):
        raise ValueError(f"packed scenes: expected [{total},2] and [{total},3], got {x.shape} and {X.shape}")
    if Kh.shape != (3, 3) and Kh.shape != (F, 3, 3):
        raise ValueError(f"K must be [3,3] or [{F},3,3], got {Kh.shape}")
    if Rh.ndim != 3 or Rh.shape[1:] != (3, 3) or Rh.shape[0] % F or th.shape != (Rh.shape[0], 3):
        raise ValueError(f"R must be [F*H,3,3] and t [F*H,3], got {Rh.shape} and {th.shape}")
    n = Rh.shape[0]
    st = None
    if status is not None:
        st = _np.ascontiguousarray(status, dtype=_np.int32)
        if st.shape != (n,):
            raise ValueError(f"status: shape {st.shape}, expected ({n},)")
    off = _np.zeros(F + 1, dtype=_np.int64)
    _np.cumsum(szs, out=off[1:])
    gain, count = _np.zeros(n, dtype=_np.float64), _np.zeros(n, dtype=_np.int32)
    L = _lib.ransac_msac_lib()
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = L.cvxpnpl_ransac_msac_score_host(F, n // F, ptr(off), total, ptr(Rh), ptr(th), ptr(st), _usable_mask(usable), ptr(Kh), int(Kh.ndim == 3),
                                          ptr(x), ptr(X), float(thresh), ptr(gain), ptr(count), int(n_threads))
    if rc != 0:
        raise RuntimeError(f"cvxpnpl_ransac_msac_score_host failed ({rc}): {L.cvxpnpl_ransac_msac_last_error().decode()}")
    return gain, count


# ---- local optimisation: the running best refitted every round (include/cvxpnpl_amd_ransac_lo.h) -----------------
# ransac_pnp_batch(confidence=..., local_opt=n) ends every round with n LO steps over the scenes still active: the correspondences that
# pass the inlier predicate at a scene's running pose are assembled into a cost (lo_assemble_active), all entries' costs are solved at the
# cost seam (solve_cost_batch), and a refitted pose that is usable and counts at least the running best is taken (lo_update_active) -- so
# the stopping rule reads the inlier share a non-minimal fit explains, not a four-point pose's.  The kernels are those of
# libcvxpnpl_amd_ransac_lo.so; the draws, the minimal solves, the round's own update and the compaction are unchanged.


def lo_thresholds(thresh: float, local_opt: int, lo_widen: float = 1.0):
    """The assembly thresholds thresh * m_k of the local_opt steps of a round, in float64 on the host:
    m_k = 1 + (lo_widen - 1) (n - 1 - k) / max(n - 1, 1) -- lo_widen * thresh in the first step, thresh in the last (and for n = 1)."""
    n, w, th = int(local_opt), float(lo_widen), float(thresh)
    return [th * (1.0 + (w - 1.0) * (n - 1 - k) / max(n - 1, 1)) for k in range(n)]


def _check_local_opt(local_opt, lo_widen, confidence, scoring):
    """Host-side validation of the LO keywords (nothing here needs a GPU).  Returns (local_opt, lo_widen)."""
    if isinstance(local_opt, bool) or not isinstance(local_opt, (int, _np.integer)) or int(local_opt) < 0:
        raise ValueError(f"local_opt must be an int >= 0, got {local_opt!r}")
    try:
        w = float(lo_widen)
    except (TypeError, ValueError):
        raise ValueError(f"lo_widen must be a finite number >= 1, got {lo_widen!r}") from None
    if not (1.0 <= w < float("inf")):  # (NaN compares false)
        raise ValueError(f"lo_widen must be a finite number >= 1, got {lo_widen!r}")
    n = int(local_opt)
    if n > 0 and confidence is None:
        raise ValueError("local_opt needs confidence=...: it refits the running best of an adaptive call (the fixed budget's LO step is refit=)")
    if n > 0 and scoring == "msac":
        raise ValueError("local_opt with scoring='msac' is not supported: a gain-based acceptance rule for refits is out of scope")
    return n, w


def _lo_cost_out(out, A, dev):
    """The (B27 [A,27], Q45 [A,45], cnt [A] int32) an LO assembly writes: allocated, or the caller's three tensors checked."""
    if out is None:
        out = (torch.empty((A, 27), dtype=torch.float64, device=dev), torch.empty((A, 45), dtype=torch.float64, device=dev),
               torch.empty((A,), dtype=torch.int32, device=dev))
    Bt, Qt, cnt = out
    _chk(Bt, "out B27", torch.float64, (A, 27), dev)
    _chk(Qt, "out Q45", torch.float64, (A, 45), dev)
    _chk(cnt, "out cnt", torch.int32, (A,), dev)
    return Bt, Qt, cnt


def _lo_update_args(sc, st, n_active, cap, confidence, fit, cnt):
    """What an LO update checks after its scenes and state: lo_taken, confidence, the active list, cap, the fit and its counts.
    Returns (A, cap, confidence)."""
    if getattr(st, "lo_taken", None) is None:
        raise ValueError("state.lo_taken is missing: the state of a call with local optimisation goes through lo_init")
    dev = sc.device
    _chk(st.lo_taken, "state.lo_taken", torch.int32, (sc.F,), dev)
    conf, _ = _check_adaptive(confidence, 1)
    A = _chk_active(sc, st.active, n_active)
    cp = int(cap)
    if not 0 <= cp <= 0x7FFFFFFF:
        raise ValueError(f"cap must be an int >= 0 (and below 2^31), got {cap!r}")
    _chk(fit.R, "fit.R", torch.float64, (A, 3, 3), dev)
    _chk(fit.t, "fit.t", torch.float64, (A, 3), dev)
    _chk(fit.status, "fit.status", torch.int32, (A,), dev)
    _chk(cnt, "cnt", torch.int32, (A,), dev)
    return A, cp, conf


def _lo_assemble_host(lib, name, F, K, R, t, active, scenes_wrong, call):
    """What the two host assemblies share once the packed scenes are arrays: K, R, t and active converted, then scenes_wrong (the
    scene-shape message, or None) and their own shapes checked in that order; the NaN / -1 outputs; call(L, ptr, act, R, t, K, B27, Q45,
    cnt) -> the return code of the entry point of L = lib(), ptr mapping an array to its pointer (None for an empty one); the raise on a
    failure."""
    import ctypes as C

    Kh = _np.ascontiguousarray(K, dtype=_np.float64)
    Rh = _np.ascontiguousarray(R, dtype=_np.float64)
    th = _np.ascontiguousarray(t, dtype=_np.float64)
    act = _np.ascontiguousarray(active, dtype=_np.int32)
    if scenes_wrong:
        raise ValueError(scenes_wrong)
    if Kh.shape != (3, 3) and Kh.shape != (F, 3, 3):
        raise ValueError(f"K must be [3,3] or [{F},3,3], got {Kh.shape}")
    if Rh.shape != (F, 3, 3) or th.shape != (F, 3):
        raise ValueError(f"R must be [{F},3,3] and t [{F},3], got {Rh.shape} and {th.shape}")
    if act.ndim != 1:
        raise ValueError(f"active must have one dimension, got shape {act.shape}")
    A = act.shape[0]
    Bt, Qt, cnt = _np.full((A, 27), _np.nan), _np.full((A, 45), _np.nan), _np.full(A, -1, dtype=_np.int32)
    ptr = lambda a: None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)  # noqa: E731
    L = lib()
    rc = call(L, ptr, act, Rh, th, Kh, Bt, Qt, cnt)
    if rc != 0:
        raise RuntimeError(f"{name}_assemble_host failed ({rc}): {getattr(L, name + '_last_error')().decode()}")
    return Bt, Qt, cnt


def lo_init(sc: Scenes, st: AdaptiveState) -> AdaptiveState:
    """cvxpnpl_ransac_lo_init: st.lo_taken [F] int32 = 0, the refits taken per scene.  Returns st."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state(sc, st)
    st.lo_taken = torch.empty((sc.F,), dtype=torch.int32, device=sc.device)
    _call("ransac_lo", sc, "cvxpnpl_ransac_lo_init", sc.F, _ptr(st.lo_taken))
    return st


def lo_assemble_active(sc: Scenes, st: AdaptiveState, n_active: int, thresh_k: float, out=None):
    """cvxpnpl_ransac_lo_assemble on the first n_active entries of st.active: (B27 [A,27], Q45 [A,45], cnt [A] int32) of the correspondences
    of scene st.active[a] that pass the inlier predicate at its running pose st.R[f], st.t[f] under thresh_k (the step's thresh * m_k,
    lo_thresholds); feed solve_cost_batch.  No mask is read or written; the sums meet in a fixed order.  Fewer than three taken: NaN, with
    the count reported.  An entry outside [0, F) leaves its rows unwritten.  out: None, or the three tensors to write into.  No
    synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state(sc, st)
    A, dev = _chk_active(sc, st.active, n_active), sc.device
    Bt, Qt, cnt = _lo_cost_out(out, A, dev)
    _call("ransac_lo", sc, "cvxpnpl_ransac_lo_assemble", sc.F, A, _ptr(st.active), _ptr(sc.offsets), sc.total, _ptr(sc.x), _ptr(sc.X), _ptr(st.R), _ptr(st.t),
          _ptr(sc.K), sc.per_scene_K, float(thresh_k), _ptr(Bt), _ptr(Qt), _ptr(cnt))
    return Bt, Qt, cnt


def lo_update_active(sc: Scenes, st: AdaptiveState, n_active: int, cap: int, confidence: float, fit, cnt, thresh: float = 2.0):
    """cvxpnpl_ransac_lo_update on the first n_active entries of st.active: the refit fit.R[a], fit.t[a], fit.status[a] of the cnt[a]
    correspondences lo_assemble_active took is counted at thresh and TAKEN when its status is 0 or 2, cnt[a] >= 4 and its count is at least
    max(st.best[f], st.head[f,1]) -- the non-minimal fit wins a tie.  Then pose, head[f,0:2], best[f] and the scene's slice of the mask
    change together, head[f,2] keeps the index of the hypothesis that seeded it and st.lo_taken[f] goes up by one.  Taken or not,
    st.done[a] |= the stopping rule at st.hyp_used[f], st.best[f].  In place, no synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    _chk_state(sc, st)
    A, cp, conf = _lo_update_args(sc, st, n_active, cap, confidence, fit, cnt)
    _call("ransac_lo", sc, "cvxpnpl_ransac_lo_update", sc.F, A, _ptr(st.active), cp, conf, _ptr(sc.offsets), sc.total, _ptr(fit.R), _ptr(fit.t),
          _ptr(fit.status), _ptr(cnt), _ptr(sc.K), sc.per_scene_K, _ptr(sc.x), _ptr(sc.X), float(thresh), _ptr(st.R), _ptr(st.t), _ptr(st.head),
          _ptr(st.best), _ptr(st.mask), _ptr(st.hyp_used), _ptr(st.lo_taken), _ptr(st.done))


def lo_assemble_host(scene_2d, scene_3d, sizes, K, R, t, active, thresh_k: float, n_threads: int = 0):
    """cvxpnpl_ransac_lo_assemble_host: what lo_assemble_active computes, on host arrays by the rules the kernel follows (the same lanes,
    the same order of the sums).  scene_2d [sum M,2], scene_3d [sum M,3] packed with sizes (F ints), K [3,3] or [F,3,3], R [F,3,3], t [F,3]
    the running poses, active: A scene indices.  Returns numpy (B27 [A,27], Q45 [A,45], cnt [A] int32); the rows of an entry outside
    [0, F) keep their initial NaN / -1.  No GPU needed."""
    szs = [int(m) for m in sizes]
    F, total = len(szs), sum(szs)
    if F < 1 or any(m < 0 for m in szs):
        raise ValueError("sizes: at least one scene, no negative size")
    x = _np.ascontiguousarray(scene_2d, dtype=_np.float64)
    X = _np.ascontiguousarray(scene_3d, dtype=_np.float64)
    wrong = None
    if x.shape != (total, 2) or X.shape != (total, 3):
        wrong = f"packed scenes: expected [{total},2] and [{total},3], got {x.shape} and {X.shape}"
    off = _np.zeros(F + 1, dtype=_np.int64)
    _np.cumsum(szs, out=off[1:])
    return _lo_assemble_host(_lib.ransac_lo_lib, "cvxpnpl_ransac_lo", F, K, R, t, active, wrong, lambda L, ptr, act, Rh, th, Kh, Bt, Qt, cnt:
                             L.cvxpnpl_ransac_lo_assemble_host(F, act.shape[0], ptr(act), ptr(off), total, ptr(x), ptr(X), ptr(Rh), ptr(th), ptr(Kh),
                                                               int(Kh.ndim == 3), float(thresh_k), ptr(Bt), ptr(Qt), ptr(cnt), int(n_threads)))


# ---- guided sampling: the best-ranked correspondences first (include/cvxpnpl_amd_ransac_guided.h) ----------------
# ransac_pnp_batch(quality=...) ranks every scene's correspondences by a matcher's score once per call and draws hypothesis h from the
# n(h) best of them; the pool grows with h (the growth function of PROSAC) and is the whole scene from h = pool_full on, where the draw is
# the uniform one again.  The kernels are those of libcvxpnpl_amd_ransac_guided.so; the stage wrappers below check every tensor as _chk does.


def pool_size(h: int, n_corr: int, pool_full: int) -> int:
    """cvxpnpl_ransac_guided_pool_host: the number of best-ranked correspondences that hypothesis h of a scene of n_corr draws from, by the
    function the sampling kernels call.  n_corr from h = pool_full on; before, min(n_T(h), 4 + h, n_corr) with n_T(h) the smallest n whose
    share pool_full * C(n,4) / C(n_corr,4) of the uniform draws reaches h + 1.  No GPU needed."""
    h, m, pf = int(h), int(n_corr), _chk_pool_full(pool_full)
    if not 0 <= h <= 0x7FFFFFFF or not 4 <= m <= 0x7FFFFFFF:
        raise ValueError(f"pool_size needs 0 <= h and 4 <= n_corr (both below 2^31), got {h}, {m}")
    return int(_lib.ransac_guided_lib().cvxpnpl_ransac_guided_pool_host(h, m, pf))


def rank_scenes(sc: Scenes, quality):
    """cvxpnpl_ransac_guided_rank: order [total] int32 from quality [total] float64 (higher is better) on the scenes' device.  Scene f's
    slice of order is a permutation of 0 .. M_f - 1, best first: j before m when its quality is greater, or equal with j < m; a NaN counts
    as -inf.  A counting rank, O(M_f^2) per scene.  No synchronisation."""
    _require_gpu()
    _chk_scenes(sc)
    _chk(quality, "quality", torch.float64, (sc.total,), sc.device)
    order = torch.empty((sc.total,), dtype=torch.int32, device=sc.device)
    _call("ransac_guided", sc, "cvxpnpl_ransac_guided_rank", sc.F, _ptr(sc.offsets), sc.total, max(sc.sizes), _ptr(quality), _ptr(order))
    return order


def sample_scenes_guided(sc: Scenes, n_hyp: int, order, pool_full: int, seeds=None, want_idx: bool = False):
    """cvxpnpl_ransac_guided_sample: what sample_scenes returns, hypothesis h of scene f drawn from the pool_size(h, M_f, pool_full) best
    entries of the scene's slice of order (rank_scenes).  pool_full = 0 is sample_scenes bit for bit.  An order entry outside [0, M_f)
    gives the NaN hypothesis with idx = -1."""
    _require_gpu()
    _chk_scenes(sc)
    H, dev, pf = int(n_hyp), sc.device, _chk_pool_full(pool_full)
    if H < 0:
        raise ValueError("n_hyp must not be negative")
    _chk(order, "order", torch.int32, (sc.total,), dev)
    sd = _seeds_dev(sc, seeds)
    p2, p3, Kh, idx = _sample_outputs(sc.F * H, sc, want_idx)
    _call("ransac_guided", sc, "cvxpnpl_ransac_guided_sample", sc.F, H, pf, _ptr(sc.offsets), sc.total, _ptr(sd), _ptr(order), _ptr(sc.x), _ptr(sc.X),
          _ptr(sc.K) if sc.per_scene_K else None, _ptr(idx), _ptr(p2), _ptr(p3), _ptr(Kh))
    return (p2, p3, Kh, idx) if want_idx else (p2, p3, Kh)


def sample_active_guided(sc: Scenes, active, n_active: int, hyp0: int, n_round: int, cap: int, order, pool_full: int, seeds=None,
                         want_idx: bool = False):
    """cvxpnpl_ransac_guided_sample_active: what sample_active returns, drawn as sample_scenes_guided draws -- the rows
    [f, hyp0 : hyp0 + n_round] of sample_scenes_guided(sc, hyp0 + n_round, order, pool_full) for f = active[a].  An entry of active outside
    [0, F) leaves its rows unwritten."""
    _require_gpu()
    _chk_scenes(sc)
    A, dev, pf = _chk_active(sc, active, n_active), sc.device, _chk_pool_full(pool_full)
    h0, Hr, cp = _chk_budget(hyp0, n_round, cap)
    _chk(order, "order", torch.int32, (sc.total,), dev)
    sd = _seeds_dev(sc, seeds)
    p2, p3, Kh, idx = _sample_outputs(A * Hr, sc, want_idx)
    _call("ransac_guided", sc, "cvxpnpl_ransac_guided_sample_active", sc.F, A, _ptr(active), h0, Hr, cp, pf, _ptr(sc.offsets), sc.total, _ptr(sd), _ptr(order),
          _ptr(sc.x), _ptr(sc.X), _ptr(sc.K) if sc.per_scene_K else None, _ptr(idx), _ptr(p2), _ptr(p3), _ptr(Kh))
    return (p2, p3, Kh, idx) if want_idx else (p2, p3, Kh)


def _check_quality(quality, pool_full, szs, packed, n_hyp):
    """Host-side validation of the guided keywords (nothing here needs a GPU): returns pool_full (None without quality; n_hyp by default)."""
    if quality is None:
        if pool_full is not None:
            raise ValueError("pool_full given without quality")
        return None
    if packed:
        sq = _shape(quality)
        if len(sq) != 1 or sq[0] != sum(szs):
            raise ValueError(f"quality: expected [{sum(szs)}] for the packed scenes, got {sq}")
    else:
        if not isinstance(quality, (list, tuple)):
            raise ValueError("quality is a list of F arrays [M_f], or packed [sum M] with `sizes`")
        if len(quality) != len(szs):
            raise ValueError(f"quality for {len(quality)} scenes, {len(szs)} scenes given")
        for f, q in enumerate(quality):
            if _shape(q) != (szs[f],):
                raise ValueError(f"scene {f}: quality {_shape(q)}, expected [{szs[f]}]")
    for q in (quality if isinstance(quality, (list, tuple)) else (quality,)):
        dt = q.dtype if hasattr(q, "dtype") else _np.asarray(q).dtype
        if (isinstance(dt, torch.dtype) and (dt.is_complex or dt == torch.bool)) or (not isinstance(dt, torch.dtype) and _np.dtype(dt).kind not in "fiu"):
            raise ValueError(f"quality must be real numbers, got dtype {dt}")
    return int(n_hyp) if pool_full is None else _chk_pool_full(pool_full)


# ---- what the two batch calls share: the first checks, the rounds of an adaptive call, and everything after the winners are known --------

def _batch_head(F, seed, n_hyp, confidence, round_hyp):
    """The first checks of a batch call after its scenes, in this order (nothing here needs a GPU): the adaptive keywords, the seeds,
    n_hyp.  Returns (seeds, confidence or None, round_hyp)."""
    conf = None
    if confidence is not None:
        conf, round_hyp = _check_adaptive(confidence, round_hyp)
    seeds = _resolve_seeds(seed, F)
    if int(n_hyp) < 1:
        raise ValueError("n_hyp must be at least 1")
    return seeds, conf, round_hyp


def _rounds(sc, st, stages, cap, conf, round_hyp, thresh, after_update=None):
    """The rounds of a batch call with confidence=... over the state st (adaptive_init / adaptive_pnpl_init): returns their number.
    stages: what differs between the scene kinds -- solve(active, n_active, hyp0, n_round), which draws the round's minimal sets and
    solves them, and the kind's score_*_active and update_*_active.  One 4-byte read-back per round -- the number of scenes still active,
    which the next round's solve needs as a host number (its batch size).  after_update(n_active), optional, runs between the round's
    update and its compaction, over the same active list: it may change the state and set st.done."""
    solve, score, update = stages
    A, h0, rounds = sc.F, 0, 0
    while A > 0 and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        res = solve(st.active, A, h0, Hr)
        count = score(sc, st.active, A, res.R, res.t, thresh, status=res.status, usable=(0, 2))
        update(sc, st, A, h0, cap, conf, count, res.R, res.t, res.status, thresh)
        if after_update is not None:
            after_update(A)
        compact_active(sc, st, A)
        A = int(st.n_active.cpu()[0])   # the round's one synchronisation
        st.swap()
        h0 += Hr
        rounds += 1
    return rounds


class _Fit:
    """What refit_update_*_scenes reads of a refit: R, t, status."""

    def __init__(self, R, t, status):
        self.R, self.t, self.status = R, t, status


def _polish(sc, refit_update, R, t, head, masks, thresh):
    """The last step of the two batch calls with polish=True: one refine_scenes launch over the consensus masks, then
    the scenes' refit_update kernel, which takes the polished pose -- with its masks and count -- only when it keeps at least the consensus
    it was fitted to.  Its candidate status is the scene's own solve status when the refinement ended CONVERGED or MAXITER, and 3 (never
    taken) otherwise.  No synchronisation.  Returns the "refine" entry of the result."""
    from .refine import refine_scenes

    res = refine_scenes(sc, R, t, mask_pts=masks[0], mask_lines=masks[1] if len(masks) > 1 else None, status=head[:, 0])
    fit = _Fit(res.R, res.t, torch.where(res.status <= 1, head[:, 0], torch.full_like(res.status, 3)))
    refit_update(sc, fit, head[:, 1].contiguous(), thresh, R, t, head, *masks)
    return {"cost": res.cost, "iters": res.iters, "status": res.status}


def _finish(sc, kind, R, t, head, masks, thresh, refit, refit_rounds, polish, n_hyp, adaptive, pool_full):
    """A batch call from the winners (R, t, head, masks) on: the refits of the consensus sets -- all scenes' in one solve at the cost seam
    --, the polish, the call's one read-back and the result.  kind: the scene kind's (assemble_*_consensus, refit_update_*_scenes, the
    result's names of the masks and of their offsets); adaptive: None or (state, rounds, confidence); pool_full: None for unguided draws."""
    assemble, refit_update, names = kind
    if refit:
        for _ in range(max(1, int(refit_rounds))):
            Bt, Qt, cnt = assemble(sc, *masks)
            fit = solve_cost_batch(Qt, Bt, eps=1e-9, max_iters=2500, device=sc.device)
            refit_update(sc, fit, cnt, thresh, R, t, head, *masks)
    refined = _polish(sc, refit_update, R, t, head, masks, thresh) if polish else None
    h = head.cpu()   # the call's one synchronisation
    out = {"R": R, "t": t}
    for (mask_name, off_name), mask, off in zip(names, masks, (sc.offsets, getattr(sc, "line_offsets", None))):
        out[mask_name], out[off_name] = mask.view(torch.bool), off
    out.update(n_inliers=h[:, 1], status=h[:, 0], n_certified=h[:, 3], best_index=h[:, 2], head=h, sizes=sc.sizes)
    if len(masks) > 1:
        out["line_sizes"] = sc.line_sizes
    out["n_hyp"] = int(n_hyp)
    if polish:
        out["refine"] = refined
    if adaptive is not None:
        state, rounds, conf = adaptive
        out.update(hyp_used=state.hyp_used.cpu(), rounds=rounds, confidence=conf)
    if pool_full is not None:
        out["pool_full"] = pool_full
    return out


def ransac_pnp_batch(pts_2d, pts_3d, K, n_hyp: int = 1024, thresh: float = 2.0, max_iters: int = 100, eps: float = 1e-6, seed=0, refit: bool = True,
                     refit_rounds: int = 1, sizes=None, device=None, polish: bool = False, confidence: Optional[float] = None, round_hyp: int = 64,
                     quality=None, pool_full: Optional[int] = None, scoring: str = "count", local_opt: int = 0, lo_widen: float = 1.0,
                     **solver_opts):
    """Robust PnP for F scenes of different sizes in one launch sequence (what ransac_pnp does for one scene per call).

    Scenes: lists of F arrays pts_2d[f] [M_f,2] / pts_3d[f] [M_f,3], or packed [sum M,2] / [sum M,3] with `sizes` (a host sequence of F
    ints).  K [3,3] or [F,3,3].  n_hyp hypotheses are drawn PER SCENE; seed is an int (scene f uses seed + f) or a sequence of F ints, and
    scene f draws exactly the minimal sets ransac_pnp(scene f, seed=seed_f, n_hyp=n_hyp) draws.
    Returns a dict: R [F,3,3], t [F,3], inliers (packed bool [sum M]) and offsets [F+1] (scene f's inliers are
    inliers[offsets[f]:offsets[f+1]]) on the device; n_inliers, status, n_certified, best_index [F] (host, columns of the one read-back
    `head` [F,4], each row what select_best's head is for one scene); sizes, n_hyp.  One host synchronisation per call.
    polish=True: after the refits the pose is refined on the pixel reprojection error of its consensus set (refine.refine_scenes) and kept
    when it holds at least that consensus; the result gains "refine": device tensors cost [F,2], iters, status [F].
    confidence (0 < confidence < 1; None: the fixed budget above, unchanged): n_hyp becomes the CAP per scene and the hypotheses are drawn
    and solved in rounds of round_hyp.  Scene f stops once it has drawn N = log(1 - confidence) / log1p(-q) hypotheses, q the chance that
    a minimal set is all inliers at the scene's best inlier count so far, or n_hyp.  A scene that stops after u hypotheses holds what the
    fixed budget n_hyp = u selects (same draws, lowest index on a tie); refits and polish then run over all scenes as above.  The result
    gains hyp_used [F] (host int32), rounds and confidence.  One 4-byte read-back per round on top of the call's own: the number of scenes
    still active is the next solve's batch size, a host number.
    quality (None: uniform draws, the code above unchanged): a matcher's score per correspondence, higher is better -- a list of F arrays
    [M_f], or packed [sum M] with `sizes`; any real dtype.  Every scene is ranked once (rank_scenes) and hypothesis h draws its minimal
    set from the pool_size(h, M_f, pool_full) best-ranked correspondences: 4 at h = 0, growing with h, the whole scene from h = pool_full
    on, where the draws are the uniform ones again.  pool_full (an int >= 0) defaults to n_hyp; 0 is the uniform sampler.  With
    confidence the stopping rule is unchanged and counts inliers of the whole scene.  The result gains pool_full.
    scoring ("count": the code above unchanged; "msac"): what selects a scene's hypothesis among its draws.  "msac" takes the highest
    gain = sum over the hypothesis' inliers of (thresh^2 - r^2) / thresh^2, i.e. the lowest truncated quadratic cost sum min(r^2, thresh^2),
    the lowest index winning an exact tie -- where many minimal sets explain all the inliers, the count ties and the gain prefers the
    pose that fits them best (score_scenes_msac, select_scenes_msac; with confidence, score_active_msac and update_active_msac, a scene
    stopping on the inlier count of its running MSAC winner).  quality / pool_full compose unchanged: they only change the draws.  The
    result of an "msac" call gains "score" ([F] float64 on the device: the gain of the selected minimal hypothesis) and "scoring"; the
    result of a "count" call is today's, key for key.  Refits and polish keep
    their acceptance rule (at least the consensus count) and their kernels; after a refit is taken, score still describes the
    hypothesis that was selected.  Out of scope: ransac_pnp (one scene, kernels of the solver library), the point-and-line calls, and a
    gain-based refit rule.
    local_opt (an int >= 0; 0: the code above unchanged, and today's result key for key; needs confidence, scoring="count"): LO-RANSAC.
    Every round ends with local_opt steps over the scenes still active: the correspondences within thresh * m_k of a scene's running
    pose are assembled into a cost (lo_assemble_active), the costs are solved at the cost seam with this call's eps / max_iters /
    solver options, and a refit of status 0 or 2, fitted to at least four correspondences, that counts -- at thresh -- at least the
    running best replaces it, a tie going to the fit (lo_update_active); the stopping rule then reads that count.  m_k falls from
    lo_widen (a float >= 1) in the first step to 1 in the last (lo_thresholds).  The draws do not depend on it, and a later round's
    minimal hypothesis replaces the running best only by a strictly higher count, so no scene draws more than without it.  Every active
    scene is refitted every round, changed or not.  The result gains lo_taken [F] (host int32: refits taken per scene), local_opt and
    lo_widen; best_index stays the index of the minimal hypothesis that seeded the running pose."""
    szs = _check_scenes(pts_2d, pts_3d, K, sizes)
    seeds, conf, round_hyp = _batch_head(len(szs), seed, n_hyp, confidence, round_hyp)
    pool_full = _check_quality(quality, pool_full, szs, sizes is not None, n_hyp)
    msac = _chk_scoring(scoring) == "msac"  # (after every earlier check: the order of their errors is pinned)
    local_opt, lo_widen = _check_local_opt(local_opt, lo_widen, confidence, scoring)
    sc = pack_scenes(pts_2d, pts_3d, K, sizes=szs if sizes is not None else None, device=device, seeds=seeds)
    guided = None
    if quality is not None:  # the ranking: once per call, before the launch sequence
        if sizes is not None and isinstance(quality, (list, tuple)):
            quality = _np.asarray(quality, dtype=_np.float64)
        guided = (rank_scenes(sc, _to_dev(quality, sc.device)), pool_full)

    def solve(p2, p3, Kh):  # the minimal solves of a fixed budget or of a round, in one launch sequence of the solver library
        return pnp_batch(p2, p3, Kh if sc.per_scene_K else sc.K, eps=eps, max_iters=max_iters, device=sc.device, **solver_opts)

    adaptive = score = None
    if conf is not None:
        cap = int(n_hyp)
        if guided is None:
            stage = lambda act, A, h0, Hr: solve(*sample_active(sc, act, A, h0, Hr, cap))  # noqa: E731
        else:
            stage = lambda act, A, h0, Hr: solve(*sample_active_guided(sc, act, A, h0, Hr, cap, *guided))  # noqa: E731
        if msac:  # the rounds with the msac stages: the round's (gain, count) travel from the score stage to the update stage as one
            state = adaptive_init_msac(sc)
            update = lambda sc_, st, A, h0, cp, cf, gc, R_, t_, s, th: update_active_msac(sc_, st, A, h0, cp, cf, gc[0], gc[1], R_, t_, s, th)  # noqa: E731
            adaptive = (state, _rounds(sc, state, (stage, score_active_msac, update), cap, conf, round_hyp, thresh), conf)
            score = state.best_gain
        elif local_opt:  # the rounds as below, each ending in local_opt refits of the running bests
            state = lo_init(sc, adaptive_init(sc))
            steps = lo_thresholds(thresh, local_opt, lo_widen)

            def lo_steps(A):
                for thresh_k in steps:
                    Bt, Qt, cnt = lo_assemble_active(sc, state, A, thresh_k)
                    fit = solve_cost_batch(Qt, Bt, eps=eps, max_iters=max_iters, device=sc.device, **solver_opts)
                    lo_update_active(sc, state, A, cap, conf, fit, cnt, thresh)

            adaptive = (state, _rounds(sc, state, (stage, score_active, update_active), cap, conf, round_hyp, thresh, after_update=lo_steps), conf)
        else:
            state = adaptive_init(sc)
            adaptive = (state, _rounds(sc, state, (stage, score_active, update_active), cap, conf, round_hyp, thresh), conf)
        R, t, head, mask = state.R, state.t, state.head, state.mask
    elif msac:  # no torch kernel from here to the read-back
        res = solve(*(sample_scenes(sc, n_hyp) if guided is None else sample_scenes_guided(sc, n_hyp, *guided)))
        gain, _ = score_scenes_msac(sc, res.R, res.t, thresh, status=res.status, usable=(0, 2))
        R, t, head, mask, score = select_scenes_msac(sc, gain, res.R, res.t, res.status, thresh)
    else:  # no torch kernel from here to the read-back
        res = solve(*(sample_scenes(sc, n_hyp) if guided is None else sample_scenes_guided(sc, n_hyp, *guided)))
        count = score_scenes(sc, res.R, res.t, thresh, status=res.status, usable=(0, 2))
        R, t, head, mask = select_scenes(sc, count, res.R, res.t, res.status, thresh)
    out = _finish(sc, (assemble_consensus, refit_update_scenes, (("inliers", "offsets"),)), R, t, head, (mask,), thresh, refit, refit_rounds,
                  polish, n_hyp, adaptive, pool_full)
    if msac:  # (the count call's result keeps exactly its keys)
        out["scoring"], out["score"] = scoring, score
    if local_opt:  # (and the call without local optimisation exactly its own)
        out.update(lo_taken=state.lo_taken.cpu(), local_opt=local_opt, lo_widen=lo_widen)
    return out


# ---- points AND lines, many scenes (include/cvxpnpl_amd_ransac_pnpl.h) --------------------------------------------
# The robust layer of pnpl: a scene is P_f point and L_f line correspondences, a minimal set is four correspondences of their union.  Its
# shape (4+0 .. 0+4) differs from hypothesis to hypothesis, and cvxpnpl_solve_batch takes one (n_p, n_l) per batch, so the sampling kernel
# assembles every hypothesis' cost itself and the F * n_hyp minimal solves go through the cost seam, as the refits do.  The kernels are
# those of libcvxpnpl_amd_ransac_pnpl.so; an inlier count is points plus lines, a line counting once.


class PnplScenes:
    """F scenes of points and lines packed on one device: x [sum P,2], X [sum P,3], l2 [sum L,2,2], l3 [sum L,2,3] float64; offsets and
    line_offsets [F+1] int64 (device); sizes, line_sizes (host tuples); K [3,3] or [F,3,3]; seeds int64 [F] on the device, or None.
    Built by pack_pnpl_scenes."""

    def __init__(self, x, X, l2, l3, offsets, line_offsets, sizes, line_sizes, K, seeds=None):
        self.x, self.X, self.l2, self.l3, self.offsets, self.line_offsets, self.K, self.seeds = x, X, l2, l3, offsets, line_offsets, K, seeds
        self.sizes, self.line_sizes = tuple(sizes), tuple(line_sizes)
        self.F, self.total, self.line_total = len(self.sizes), int(sum(self.sizes)), int(sum(self.line_sizes))
        self.per_scene_K, self.device = int(K.dim() == 3), K.device


def _numel(a):
    n = 1
    for s in _shape(a):
        n *= int(s)
    return n


def _pair_sizes(a2, a3, sizes, what, tail2, tail3):
    """Sizes of one kind of correspondence (points or lines) over the scenes, or None when the pair is absent.  tail2 / tail3: the shape
    of one 2D / 3D record.  A scene's entry may be None or empty."""
    if a2 is None and a3 is None:
        if sizes is not None and any(int(s) for s in sizes):
            raise ValueError(f"sizes of {what} given without {what}")
        return None
    if a2 is None or a3 is None:
        raise ValueError(f"{what}: the 2D and the 3D half go together")
    if sizes is None:
        if not isinstance(a2, (list, tuple)) or not isinstance(a3, (list, tuple)):
            raise ValueError(f"{what}: scenes are a list of F 2D arrays and a list of F 3D arrays, or packed arrays with their sizes")
        if len(a2) != len(a3):
            raise ValueError(f"{len(a2)} scenes of 2D {what} for {len(a3)} scenes of 3D {what}")
        out = []
        for f, (a, b) in enumerate(zip(a2, a3)):
            na = 0 if a is None or _numel(a) == 0 else None
            nb = 0 if b is None or _numel(b) == 0 else None
            if na is None:
                sa = _shape(a)
                if len(sa) != 1 + len(tail2) or sa[1:] != tail2:
                    raise ValueError(f"scene {f}: expected 2D {what} [n,{','.join(map(str, tail2))}], got {sa}")
                na = int(sa[0])
            if nb is None:
                sb = _shape(b)
                if len(sb) != 1 + len(tail3) or sb[1:] != tail3:
                    raise ValueError(f"scene {f}: expected 3D {what} [n,{','.join(map(str, tail3))}], got {sb}")
                nb = int(sb[0])
            if na != nb:
                raise ValueError(f"scene {f}: {na} 2D {what} for {nb} 3D {what}")
            out.append(na)
        return out
    out = [int(s) for s in sizes]
    if any(s < 0 for s in out):
        raise ValueError(f"negative size among the sizes of {what}")
    sa, sb = _shape(a2), _shape(a3)
    na = 0 if _numel(a2) == 0 else None
    nb = 0 if _numel(a3) == 0 else None
    if na is None:
        if len(sa) != 1 + len(tail2) or sa[1:] != tail2:
            raise ValueError(f"packed scenes: expected 2D {what} [n,{','.join(map(str, tail2))}], got {sa}")
        na = int(sa[0])
    if nb is None:
        if len(sb) != 1 + len(tail3) or sb[1:] != tail3:
            raise ValueError(f"packed scenes: expected 3D {what} [n,{','.join(map(str, tail3))}], got {sb}")
        nb = int(sb[0])
    if na != nb:
        raise ValueError(f"packed scenes: {na} 2D {what} for {nb} 3D {what}")
    if sum(out) != na:
        raise ValueError(f"sizes add up to {sum(out)}, the packed scenes hold {na} {what}")
    return out


def _check_pnpl_scenes(pts_2d, line_2d, pts_3d, line_3d, K, sizes, line_sizes):
    """Host-side validation of a scene set of points and lines (nothing here needs a GPU): returns (sizes, line_sizes).  ValueError for an
    empty set, a scene of fewer than four correspondences in total, 2D / 3D lengths that differ (points or lines), different numbers of
    point scenes and line scenes, sizes that do not add up, or a K that is neither [3,3] nor [F,3,3]."""
    ps = _pair_sizes(pts_2d, pts_3d, sizes, "points", (2,), (3,))
    ls = _pair_sizes(line_2d, line_3d, line_sizes, "lines", (2, 2), (2, 3))
    if ps is None and ls is None:
        raise ValueError("no scenes: neither points nor lines")
    if ps is not None and ls is not None and len(ps) != len(ls):
        raise ValueError(f"{len(ps)} scenes of points for {len(ls)} scenes of lines")
    F = len(ps if ps is not None else ls)
    ps = [0] * F if ps is None else ps
    ls = [0] * F if ls is None else ls
    if F == 0:
        raise ValueError("no scenes")
    for f in range(F):
        if ps[f] + ls[f] < 4:
            raise ValueError(f"scene {f} has {ps[f]} points and {ls[f]} lines: a minimal set needs 4 correspondences")
    sk = _shape(K)
    if sk != (3, 3) and sk != (F, 3, 3):
        raise ValueError(f"K must be [3,3] or [{F},3,3], got {sk}")
    return ps, ls


def _pack_half(a, tail, device):
    """One packed correspondence array [n, *tail] on the device from a list of per-scene arrays (None / empty entries dropped), a packed
    array, or None."""
    if isinstance(a, (list, tuple)):
        a = [b for b in a if b is not None and _numel(b) > 0]
        if a and any(isinstance(b, torch.Tensor) for b in a):
            return torch.cat([torch.as_tensor(b, dtype=torch.float64, device=device).reshape((-1,) + tail) for b in a]).contiguous()
        a = _np.concatenate([_np.asarray(b, dtype=_np.float64).reshape((-1,) + tail) for b in a]) if a else None
    if a is None or _numel(a) == 0:
        return torch.zeros((0,) + tail, dtype=torch.float64, device=device)
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(_np.ascontiguousarray(a, dtype=_np.float64))
    return a.to(device=device, dtype=torch.float64).reshape((-1,) + tail).contiguous()


def pack_pnpl_scenes(pts_2d, line_2d, pts_3d, line_3d, K, sizes=None, line_sizes=None, device=None, seeds=None) -> PnplScenes:
    """Validate (on the host) and pack a scene set of points and lines on the device; the argument order is pnpl's.  pts_2d / pts_3d: lists
    of F arrays [P_f,2] / [P_f,3], or packed with `sizes`; line_2d / line_3d: lists of F arrays [L_f,2,2] / [L_f,2,3], or packed with
    `line_sizes`.  Either pair may be None or empty, for all scenes or for single ones.  K [3,3] or [F,3,3].  seeds (optional, F ints):
    both offset arrays and the seeds travel in ONE host-to-device copy."""
    ps, ls = _check_pnpl_scenes(pts_2d, line_2d, pts_3d, line_3d, K, sizes, line_sizes)
    F = len(ps)
    if seeds is not None and len(seeds) != F:
        raise ValueError(f"{len(seeds)} seeds for {F} scenes")
    _require_gpu()
    device = _pick_device(device, pts_3d, line_3d, pts_2d, line_2d, K)
    meta = _np.zeros(2 * (F + 1) + (F if seeds is not None else 0), dtype=_np.int64)  # both offset arrays, then the seeds: one copy
    _np.cumsum(ps, out=meta[1:F + 1])
    _np.cumsum(ls, out=meta[F + 2:2 * F + 2])
    if seeds is not None:
        meta[2 * F + 2:] = _seed_words(seeds)
    meta = torch.as_tensor(meta).to(device)
    sd = meta[2 * F + 2:] if seeds is not None else None
    Kd = K if isinstance(K, torch.Tensor) else torch.as_tensor(_np.ascontiguousarray(K, dtype=_np.float64))
    return PnplScenes(_pack_half(pts_2d, (2,), device), _pack_half(pts_3d, (3,), device), _pack_half(line_2d, (2, 2), device),
                      _pack_half(line_3d, (2, 3), device), meta[:F + 1], meta[F + 1:2 * F + 2], ps, ls, _to_dev(Kd, device), sd)


def sample_assemble_scenes(sc: PnplScenes, n_hyp: int, seeds=None, want_idx: bool = False):
    """cvxpnpl_ransac_pnpl_sample_assemble: n_hyp minimal sets per scene, drawn over the union of the scene's points and lines (index c <
    P_f: point c; otherwise line c - P_f; scene f draws what synth.philox_minimal_sets(n_hyp, P_f + L_f, 4, seeds[f]) draws) and
    assembled in place.  Returns (Q45 [F*n_hyp,45], B27 [F*n_hyp,27]), the inputs of solve_cost_batch, and with want_idx idx [F*n_hyp,4]
    int32.  seeds: a sequence of F ints (None: the seeds packed with the scenes)."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    H, dev = int(n_hyp), sc.device
    if H < 0:
        raise ValueError("n_hyp must not be negative")
    sd = _seeds_dev(sc, seeds, "pack_pnpl_scenes")
    Qt, Bt, idx = _cost_outputs(sc.F * H, dev, want_idx)
    _call("ransac_pnpl", sc, "cvxpnpl_ransac_pnpl_sample_assemble", sc.F, H, *_scene_args(sc), _ptr(sd), *_data_args(sc), _ptr(sc.K), sc.per_scene_K, _ptr(idx),
          _ptr(Qt), _ptr(Bt))
    return (Qt, Bt, idx) if want_idx else (Qt, Bt)


def score_pnpl_scenes(sc: PnplScenes, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_pnpl_score: count [F*H] int32, the point plus line inliers of hypothesis (f, h) = (R, t)[f*H + h] in scene f."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    H = _poses(sc, R, t, status, None, sc.F, "R must be [F*H,3,3]", min_one=False)
    count = torch.empty((sc.F * H,), dtype=torch.int32, device=sc.device)
    _call("ransac_pnpl", sc, "cvxpnpl_ransac_pnpl_score", sc.F, H, *_scene_args(sc), _ptr(R), _ptr(t), _ptr(status), _usable_mask(usable), _ptr(sc.K),
          sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(count))
    return count


def select_pnpl_scenes(sc: PnplScenes, count, R, t, status, thresh: float = 2.0):
    """cvxpnpl_ransac_pnpl_select: per scene the hypothesis of the highest count (lowest index on a tie).  Returns R [F,3,3], t [F,3],
    head [F,4] int32 = (status, inliers, index within the scene, certified hypotheses), mask_pts [sum P] and mask_lines [sum L] uint8.
    No synchronisation."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    H, dev = _poses(sc, R, t, status, count, sc.F, "R must be [F*H,3,3] with H >= 1", required=True), sc.device
    oR = torch.empty((sc.F, 3, 3), dtype=torch.float64, device=dev)
    ot = torch.empty((sc.F, 3), dtype=torch.float64, device=dev)
    head = torch.empty((sc.F, 4), dtype=torch.int32, device=dev)
    mp = torch.empty((sc.total,), dtype=torch.uint8, device=dev)
    ml = torch.empty((sc.line_total,), dtype=torch.uint8, device=dev)
    _call("ransac_pnpl", sc, "cvxpnpl_ransac_pnpl_select", sc.F, H, *_scene_args(sc), _ptr(count), _ptr(R), _ptr(t), _ptr(status), _ptr(sc.K),
          sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(oR), _ptr(ot), _ptr(head), _ptr(mp), _ptr(ml))
    return oR, ot, head, mp, ml


def assemble_pnpl_consensus(sc: PnplScenes, mask_pts, mask_lines):
    """cvxpnpl_ransac_pnpl_assemble_consensus: (B27 [F,27], Q45 [F,45], count [F] int32) of every scene's masked points and lines (uint8
    masks [sum P] / [sum L], non-zero = taken); feed solve_cost_batch.  Fewer than three correspondences taken: NaN for that scene."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    dev = sc.device
    _chk(mask_pts, "mask_pts", torch.uint8, (sc.total,), dev)
    _chk(mask_lines, "mask_lines", torch.uint8, (sc.line_total,), dev)
    Bt = torch.empty((sc.F, 27), dtype=torch.float64, device=dev)
    Qt = torch.empty((sc.F, 45), dtype=torch.float64, device=dev)
    cnt = torch.empty((sc.F,), dtype=torch.int32, device=dev)
    _call("ransac_pnpl", sc, "cvxpnpl_ransac_pnpl_assemble_consensus", sc.F, *_scene_args(sc), *_data_args(sc), _ptr(mask_pts), _ptr(mask_lines), _ptr(sc.K),
          sc.per_scene_K, _ptr(Bt), _ptr(Qt), _ptr(cnt))
    return Bt, Qt, cnt


def refit_update_pnpl_scenes(sc: PnplScenes, fit, fit_count, thresh, R, t, head, mask_pts, mask_lines):
    """cvxpnpl_ransac_pnpl_refit_update: per scene, take the refitted pose fit.R[f] / fit.t[f] -- pose, status, both masks and count
    together, in place -- when it is usable and keeps at least head[f,1] inliers.  One launch, no synchronisation."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    dev = _chk_refit(sc, fit, fit_count, R, t, head)
    _chk(mask_pts, "mask_pts", torch.uint8, (sc.total,), dev)
    _chk(mask_lines, "mask_lines", torch.uint8, (sc.line_total,), dev)
    _call("ransac_pnpl", sc, "cvxpnpl_ransac_pnpl_refit_update", sc.F, *_scene_args(sc), _ptr(fit.R), _ptr(fit.t), _ptr(fit.status), _ptr(fit_count),
          _ptr(sc.K), sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(R), _ptr(t), _ptr(head), _ptr(mask_pts), _ptr(mask_lines))


# The cost seam does not tell the solver how many correspondences stand behind a cost, and its launch plan then assumes a well
# over-determined problem: the interior-point path for slowly converging problems starts after 128 iterations, beyond the 100 a
# hypothesis is given.  Minimal problems are the slow ones (a fifth is still open after 32 iterations), and
# cvxpnpl_solve_batch hands four-correspondence problems over after 32; the minimal solves here ask for the same.
MINIMAL_SOLVER_OPTS = {"rescue_from": 32}


def solve_minimal_costs(Q45, B27, eps: float = 1e-6, max_iters: int = 100, device=None, **solver_opts):
    """solve_cost_batch on the costs of minimal sets (sample_assemble_scenes), with MINIMAL_SOLVER_OPTS unless the caller overrides them."""
    return solve_cost_batch(Q45, B27, eps=eps, max_iters=max_iters, device=device, **{**MINIMAL_SOLVER_OPTS, **solver_opts})


# ---- points AND lines with a budget per scene and ranked draws (include/cvxpnpl_amd_ransac_pnpl_adaptive.h) --------
# ransac_pnpl_batch(confidence=..., quality=..., line_quality=...): the rounds of section 19 and the ranked draws of section 20 over the
# UNION of a scene's points and lines (index c < P_f: point c; otherwise line c - P_f; M_f = P_f + L_f).  The start of a call, the
# compaction and the ranking are the ninth and tenth libraries', which know nothing of what a correspondence is; the three kernels that
# touch points and lines are those of libcvxpnpl_amd_ransac_pnpl_adaptive.so.  The stage wrappers below check every tensor as _chk does.


def adaptive_pnpl_init(sc: PnplScenes) -> AdaptiveState:
    """adaptive_init for scenes of points and lines: the state of section 19 (cvxpnpl_ransac_adaptive_init, which reads nothing of a
    scene), its mask the POINT mask [sum P], and beside it mask_lines [sum L] uint8."""
    _chk_pnpl_scenes(sc)
    st = adaptive_init(sc)
    st.mask_lines = torch.empty((sc.line_total,), dtype=torch.uint8, device=sc.device)
    return st


def rank_pnpl_scenes(sc: PnplScenes, quality, line_quality):
    """The ranking of a guided call: order [sum P + sum L] int32, scene f's slice -- from offsets[f] + line_offsets[f] on -- the union
    indices of its correspondences, best first, by cvxpnpl_ransac_guided_rank (rank_scenes) over the union offsets and the union-packed
    quality (per scene: points, then lines).  quality [sum P], line_quality [sum L]: float64 on the scenes' device, on ONE scale; either
    may be None where the scene set has no such correspondence.  No synchronisation."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    dev, n = sc.device, sc.total + sc.line_total
    union = torch.empty((n,), dtype=torch.float64, device=dev)
    off_p, off_l = _np.concatenate([[0], _np.cumsum(sc.sizes)]), _np.concatenate([[0], _np.cumsum(sc.line_sizes)])
    if sc.total:  # point m of scene f sits at its packed place plus the lines of the scenes before it ...
        _chk(quality, "quality", torch.float64, (sc.total,), dev)
        union[torch.as_tensor(_np.arange(sc.total) + _np.repeat(off_l[:-1], sc.sizes)).to(dev)] = quality
    if sc.line_total:  # ... and line m at its packed place plus the points of the scenes up to its own
        _chk(line_quality, "line_quality", torch.float64, (sc.line_total,), dev)
        union[torch.as_tensor(_np.arange(sc.line_total) + _np.repeat(off_p[1:], sc.line_sizes)).to(dev)] = line_quality
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    _call("ransac_guided", sc, "cvxpnpl_ransac_guided_rank", sc.F, _ptr((sc.offsets + sc.line_offsets).contiguous()), n,
          max(p + l for p, l in zip(sc.sizes, sc.line_sizes)), _ptr(union), _ptr(order))
    return order


def sample_assemble_active(sc: PnplScenes, active, n_active: int, hyp0: int, n_round: int, cap: int, order=None, pool_full: int = 0, seeds=None,
                           want_idx: bool = False):
    """cvxpnpl_ransac_pnpl_adaptive_sample_assemble: for entry a < n_active of `active`, the hypotheses hyp0 .. hyp0 + n_round - 1 of scene
    active[a], drawn and assembled as sample_assemble_scenes does -- without order (or with pool_full = 0) the rows
    [f, hyp0 : hyp0 + n_round] of sample_assemble_scenes(sc, hyp0 + n_round), bit for bit.  order (rank_pnpl_scenes) with pool_full > 0:
    hypothesis h of the scene draws from the pool_size(h, P_f + L_f, pool_full) best-ranked correspondences of the union while
    h < pool_full.  Returns (Q45 [A*n_round,45], B27 [A*n_round,27]) and, with want_idx, idx [A*n_round,4] int32 (union indices).  An
    entry of active outside [0, F) leaves its rows unwritten; an order entry outside [0, M_f) gives the NaN cost with idx = -1."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    A, dev, pf = _chk_active(sc, active, n_active), sc.device, _chk_pool_full(pool_full)
    h0, Hr, cp = _chk_budget(hyp0, n_round, cap)
    if order is None:
        if pf > 0:
            raise ValueError("pool_full > 0 needs order (rank_pnpl_scenes)")
    else:
        _chk(order, "order", torch.int32, (sc.total + sc.line_total,), dev)
    sd = _seeds_dev(sc, seeds, "pack_pnpl_scenes")
    Qt, Bt, idx = _cost_outputs(A * Hr, dev, want_idx)
    _call("ransac_pnpl_adaptive", sc, "cvxpnpl_ransac_pnpl_adaptive_sample_assemble", sc.F, A, _ptr(active), h0, Hr, cp, pf, *_scene_args(sc), _ptr(sd),
          _ptr(order), *_data_args(sc), _ptr(sc.K), sc.per_scene_K, _ptr(idx), _ptr(Qt), _ptr(Bt))
    return (Qt, Bt, idx) if want_idx else (Qt, Bt)


def score_pnpl_active(sc: PnplScenes, active, n_active: int, R, t, thresh: float = 2.0, status=None, usable=(0, 2)):
    """cvxpnpl_ransac_pnpl_adaptive_score: count [A*n_round] int32, the point plus line inliers of (R, t)[a*n_round + h] in scene
    active[a]; predicates and status rule of score_pnpl_scenes."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    A = _chk_active(sc, active, n_active)
    Hr = _chk_round(sc, A, R, t, status)
    count = torch.empty((A * Hr,), dtype=torch.int32, device=sc.device)
    _call("ransac_pnpl_adaptive", sc, "cvxpnpl_ransac_pnpl_adaptive_score", sc.F, A, _ptr(active), Hr, *_scene_args(sc), _ptr(R), _ptr(t), _ptr(status),
          _usable_mask(usable), _ptr(sc.K), sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(count))
    return count


def update_pnpl_active(sc: PnplScenes, st: AdaptiveState, n_active: int, hyp0: int, cap: int, confidence: float, count, R, t, status,
                       thresh: float = 2.0):
    """cvxpnpl_ransac_pnpl_adaptive_update on the first n_active entries of st.active (a state of adaptive_pnpl_init): update_active with
    two masks -- st.mask (points) and st.mask_lines change together with pose, head and best -- and the stopping rule on P_f + L_f.
    n_round is R.shape[0] / n_active.  In place, no synchronisation; compact_active(sc, st, n_active) follows."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    _chk_state(sc, st)
    _chk(getattr(st, "mask_lines", None), "state.mask_lines", torch.uint8, (sc.line_total,), sc.device)
    conf, _ = _check_adaptive(confidence, 1)
    A = _chk_active(sc, st.active, n_active)
    if status is None:
        raise ValueError("status is required")
    Hr = _chk_round(sc, A, R, t, status, count)
    h0, Hr, cp = _chk_budget(hyp0, Hr, cap)
    _call("ransac_pnpl_adaptive", sc, "cvxpnpl_ransac_pnpl_adaptive_update", sc.F, A, _ptr(st.active), h0, Hr, cp, conf, *_scene_args(sc), _ptr(count), _ptr(R),
          _ptr(t), _ptr(status), _ptr(sc.K), sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(st.R), _ptr(st.t), _ptr(st.head),
          _ptr(st.best), _ptr(st.mask), _ptr(st.mask_lines), _ptr(st.hyp_used), _ptr(st.done))

# ---- local optimisation for points AND lines (include/cvxpnpl_amd_ransac_pnpl_lo.h) -------------------------------
# ransac_pnpl_batch(confidence=..., local_opt=n): the LO steps of section 24 over the union of a scene's points and lines.  The state is
# adaptive_pnpl_init's plus lo_init's counter (the fourteenth library's kernel, which reads nothing of a scene); the two kernels that
# touch points and lines are those of libcvxpnpl_amd_ransac_pnpl_lo.so.


def _chk_pnpl_lo_state(sc, st):
    _chk_state(sc, st)
    _chk(getattr(st, "mask_lines", None), "state.mask_lines", torch.uint8, (sc.line_total,), sc.device)


def lo_assemble_pnpl_active(sc: PnplScenes, st: AdaptiveState, n_active: int, thresh_k: float, out=None):
    """cvxpnpl_ransac_pnpl_lo_assemble on the first n_active entries of st.active: (B27 [A,27], Q45 [A,45], cnt [A] int32) of the points
    of scene st.active[a] that pass the point predicate and of its lines that pass the line predicate -- both end points in front of the
    camera and within thresh_k pixels of the image line -- at the running pose st.R[f], st.t[f] under thresh_k (the step's
    thresh * m_k, lo_thresholds); cnt counts points plus lines, a line once; feed solve_cost_batch.  No mask is read or written; the sums
    meet in a fixed order (a lane's points, then its lines) about the centre of the first three taken 3D records, points first.  Fewer
    than three taken: NaN, with the count reported.  An entry outside [0, F) leaves its rows unwritten.  out: None, or the three tensors
    to write into.  No synchronisation."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    _chk_pnpl_lo_state(sc, st)
    A, dev = _chk_active(sc, st.active, n_active), sc.device
    Bt, Qt, cnt = _lo_cost_out(out, A, dev)
    _call("ransac_pnpl_lo", sc, "cvxpnpl_ransac_pnpl_lo_assemble", sc.F, A, _ptr(st.active), *_scene_args(sc), *_data_args(sc), _ptr(st.R), _ptr(st.t),
          _ptr(sc.K), sc.per_scene_K, float(thresh_k), _ptr(Bt), _ptr(Qt), _ptr(cnt))
    return Bt, Qt, cnt


def lo_update_pnpl_active(sc: PnplScenes, st: AdaptiveState, n_active: int, cap: int, confidence: float, fit, cnt, thresh: float = 2.0):
    """cvxpnpl_ransac_pnpl_lo_update on the first n_active entries of st.active: lo_update_active with two masks.  The refit fit.R[a],
    fit.t[a], fit.status[a] of the cnt[a] correspondences lo_assemble_pnpl_active took is counted at thresh over the scene's points and
    lines and TAKEN when its status is 0 or 2, cnt[a] >= 4 and its count is at least max(st.best[f], st.head[f,1]) -- the non-minimal fit
    wins a tie.  Then pose, head[f,0:2], best[f], the scene's slice of st.mask (points) and its slice of st.mask_lines change together,
    head[f,2] stays and st.lo_taken[f] goes up by one.  Taken or not, st.done[a] |= the stopping rule at st.hyp_used[f], st.best[f] over
    P_f + L_f.  In place, no synchronisation."""
    _require_gpu()
    _chk_pnpl_scenes(sc)
    _chk_pnpl_lo_state(sc, st)
    A, cp, conf = _lo_update_args(sc, st, n_active, cap, confidence, fit, cnt)
    _call("ransac_pnpl_lo", sc, "cvxpnpl_ransac_pnpl_lo_update", sc.F, A, _ptr(st.active), cp, conf, *_scene_args(sc), _ptr(fit.R), _ptr(fit.t),
          _ptr(fit.status), _ptr(cnt), _ptr(sc.K), sc.per_scene_K, *_data_args(sc), float(thresh), _ptr(st.R), _ptr(st.t), _ptr(st.head),
          _ptr(st.best), _ptr(st.mask), _ptr(st.mask_lines), _ptr(st.hyp_used), _ptr(st.lo_taken), _ptr(st.done))


def lo_assemble_pnpl_host(pts_2d, pts_3d, line_2d, line_3d, sizes, line_sizes, K, R, t, active, thresh_k: float, n_threads: int = 0):
    """cvxpnpl_ransac_pnpl_lo_assemble_host: what lo_assemble_pnpl_active computes, on host arrays by the rules the kernel follows (the
    same lanes, the same order of the sums).  pts_2d [sum P,2], pts_3d [sum P,3] packed with sizes, line_2d [sum L,2,2], line_3d
    [sum L,2,3] packed with line_sizes (F ints each; a half may be None or empty), K [3,3] or [F,3,3], R [F,3,3], t [F,3] the running
    poses, active: A scene indices.  Returns numpy (B27 [A,27], Q45 [A,45], cnt [A] int32); the rows of an entry outside [0, F) keep
    their initial NaN / -1.  No GPU needed."""
    ps, ls = [int(m) for m in sizes], [int(m) for m in line_sizes]
    F, nP, nL = len(ps), sum(ps), sum(ls)
    if F < 1 or len(ls) != F or any(m < 0 for m in ps + ls):
        raise ValueError("sizes and line_sizes: at least one scene, as many of one as of the other, no negative size")
    x = _np.ascontiguousarray(_np.zeros((0, 2)) if pts_2d is None else pts_2d, dtype=_np.float64).reshape(-1, 2)
    X = _np.ascontiguousarray(_np.zeros((0, 3)) if pts_3d is None else pts_3d, dtype=_np.float64).reshape(-1, 3)
    l2 = _np.ascontiguousarray(_np.zeros((0, 2, 2)) if line_2d is None else line_2d, dtype=_np.float64).reshape(-1, 2, 2)
    l3 = _np.ascontiguousarray(_np.zeros((0, 2, 3)) if line_3d is None else line_3d, dtype=_np.float64).reshape(-1, 2, 3)
    wrong = None
    if x.shape[0] != nP or X.shape[0] != nP:
        wrong = f"packed points: expected [{nP},2] and [{nP},3], got {x.shape} and {X.shape}"
    elif l2.shape[0] != nL or l3.shape[0] != nL:
        wrong = f"packed lines: expected [{nL},2,2] and [{nL},2,3], got {l2.shape} and {l3.shape}"
    off_p, off_l = _np.zeros(F + 1, dtype=_np.int64), _np.zeros(F + 1, dtype=_np.int64)
    _np.cumsum(ps, out=off_p[1:])
    _np.cumsum(ls, out=off_l[1:])
    return _lo_assemble_host(_lib.ransac_pnpl_lo_lib, "cvxpnpl_ransac_pnpl_lo", F, K, R, t, active, wrong, lambda L, ptr, act, Rh, th, Kh, Bt, Qt, cnt:
                             L.cvxpnpl_ransac_pnpl_lo_assemble_host(F, act.shape[0], ptr(act), ptr(off_p), nP, ptr(off_l), nL, ptr(x), ptr(X), ptr(l2),
                                                                    ptr(l3), ptr(Rh), ptr(th), ptr(Kh), int(Kh.ndim == 3), float(thresh_k), ptr(Bt),
                                                                    ptr(Qt), ptr(cnt), int(n_threads)))


def _check_pnpl_quality(quality, line_quality, pool_full, ps, ls, packed_p, packed_l, n_hyp):
    """Host-side validation of the guided keywords of ransac_pnpl_batch (nothing here needs a GPU): returns pool_full (None for an
    unguided call; n_hyp by default).  A guided call gives a quality for every kind of correspondence the scene set holds."""
    if quality is None and line_quality is None:
        if pool_full is not None:
            raise ValueError("pool_full given without quality")
        return None
    for q, szs, what, other in ((quality, ps, "quality", "points"), (line_quality, ls, "line_quality", "lines")):
        if q is None and sum(szs):
            raise ValueError(f"a guided call ranks points and lines together: the scenes hold {other}, {what} is missing")
        if q is not None and not sum(szs):
            raise ValueError(f"{what} given, the scenes hold no {other}")
    pf = int(n_hyp) if pool_full is None else _chk_pool_full(pool_full)
    for q, szs, packed, what in ((quality, ps, packed_p, "quality"), (line_quality, ls, packed_l, "line_quality")):
        if q is None:
            continue
        if not packed and isinstance(q, (list, tuple)):  # a scene without this kind may give None
            q = [_np.zeros(0) if a is None else a for a in q]
        try:
            _check_quality(q, 0, szs, packed, n_hyp)
        except ValueError as e:
            raise ValueError(str(e).replace("quality", what)) from None
    return pf


def _pack_quality(q, packed, device):
    """One kind's quality as float64 [n] on the device (None stays None)."""
    if q is None:
        return None
    if isinstance(q, (list, tuple)):
        q = _np.asarray(q, dtype=_np.float64) if packed else [a for a in q if a is not None and _numel(a) > 0]
    return _to_dev(q, device).reshape(-1)


def ransac_pnpl_batch(pts_2d, line_2d, pts_3d, line_3d, K, n_hyp: int = 1024, thresh: float = 2.0, max_iters: int = 100, eps: float = 1e-6, seed=0,
                      refit: bool = True, refit_rounds: int = 1, sizes=None, line_sizes=None, device=None, polish: bool = False,
                      confidence: Optional[float] = None, round_hyp: int = 64, quality=None, line_quality=None, pool_full: Optional[int] = None,
                      local_opt: int = 0, lo_widen: float = 1.0, **solver_opts):
    """Robust PnPL for F scenes of different sizes in one launch sequence; the argument order is pnpl's.

    Scenes: lists of F arrays pts_2d[f] [P_f,2] / pts_3d[f] [P_f,3] / line_2d[f] [L_f,2,2] / line_3d[f] [L_f,2,3], or packed arrays with
    `sizes` / `line_sizes` (host sequences of F ints).  Either pair may be None or empty, for all scenes or for single ones; a scene needs
    P_f + L_f >= 4.  K [3,3] or [F,3,3].  n_hyp minimal sets of four correspondences are drawn PER SCENE from the union of its points and
    lines; seed is an int (scene f uses seed + f) or a sequence of F ints.  A point is an inlier when it reprojects within thresh pixels in
    front of the camera, a line when both projected end points lie within thresh pixels of its image line, in front of the camera.
    Returns a dict: R [F,3,3], t [F,3], inliers_pts (packed bool [sum P]) with offsets [F+1], inliers_lines (packed bool [sum L]) with
    line_offsets [F+1] on the device; n_inliers (points + lines, a line counting once), status, n_certified, best_index [F] (host, columns
    of the one read-back `head` [F,4]); sizes, line_sizes, n_hyp.  One host synchronisation per call.
    polish=True: as in ransac_pnp_batch, over both consensus masks; the result gains "refine".
    confidence (0 < confidence < 1; None: the fixed budget above, unchanged), round_hyp: as in ransac_pnp_batch, on the UNION of a scene's
    correspondences -- n_hyp becomes the CAP per scene, the hypotheses are drawn, assembled, solved and scored in rounds of round_hyp for
    the scenes still active, and scene f stops once it has drawn N(best, P_f + L_f, confidence) hypotheses (needed_hypotheses), best its
    highest inlier count so far (points plus lines), or n_hyp.  A scene that stops after u hypotheses holds what the fixed budget
    n_hyp = u selects; refits and polish then run over all scenes.  The result gains hyp_used [F] (host int32), rounds and confidence.
    One 4-byte read-back per round on top of the call's own.
    quality / line_quality (None: uniform draws, the code above unchanged): a matcher's score per point / per line, higher is better --
    lists of F arrays [P_f] / [L_f] (None for a scene without that kind), or packed [sum P] / [sum L] with `sizes` / `line_sizes`; any
    real dtype.  A guided call gives one for every kind of correspondence the scenes hold.  The two are compared ON ONE SCALE: points and
    lines are ranked together, and making a point score comparable with a line score is the caller's contract.  Every scene's union is
    ranked once (rank_pnpl_scenes) and hypothesis h draws its minimal set from the pool_size(h, P_f + L_f, pool_full) best-ranked
    correspondences while h < pool_full; from there on the draws are the uniform ones.  pool_full (an int >= 0) defaults to n_hyp; 0 is
    the uniform sampler bit for bit.  With confidence the stopping rule is unchanged and counts inliers of the whole scene.  The result
    gains pool_full.
    local_opt (an int >= 0; 0: the code above unchanged, and today's result key for key; needs confidence): LO-RANSAC as in
    ransac_pnp_batch, on the UNION of a scene's points and lines.  Every round ends with local_opt steps over the scenes still active:
    the points and lines within thresh * m_k of a scene's running pose are assembled into a cost (lo_assemble_pnpl_active), the costs
    are solved by solve_cost_batch with this call's eps / max_iters / solver options, and a refit of status 0 or 2, fitted to at least
    four correspondences, that counts -- at thresh, points plus lines -- at least the running best replaces it, a tie going to the fit
    (lo_update_pnpl_active); the stopping rule then reads that count.  The refits do NOT go through solve_minimal_costs:
    MINIMAL_SOLVER_OPTS exists for the costs of four correspondences, and a consensus set is over-determined -- the case the solver's
    launch plan assumes at the cost seam.  m_k falls from lo_widen (a float >= 1) in the first step to 1 in the last (lo_thresholds).
    The draws do not depend on it, and a later round's minimal hypothesis replaces the running best only by a strictly higher count, so
    no scene draws more than without it.  quality / line_quality compose unchanged: they only change the draws.  The result gains
    lo_taken [F] (host int32: refits taken per scene), local_opt and lo_widen; best_index stays the index of the minimal hypothesis
    that seeded the running pose."""
    ps, ls = _check_pnpl_scenes(pts_2d, line_2d, pts_3d, line_3d, K, sizes, line_sizes)
    F = len(ps)
    seeds, conf, round_hyp = _batch_head(F, seed, n_hyp, confidence, round_hyp)
    pool_full = _check_pnpl_quality(quality, line_quality, pool_full, ps, ls, sizes is not None, line_sizes is not None, n_hyp)
    local_opt, lo_widen = _check_local_opt(local_opt, lo_widen, confidence, "count")  # (after every earlier check: the order of their errors is pinned)
    sc = pack_pnpl_scenes(pts_2d, line_2d, pts_3d, line_3d, K, sizes=sizes, line_sizes=line_sizes, device=device, seeds=seeds)
    order = None
    if pool_full is not None:  # the ranking of every scene's union: once per call, before the launch sequence
        order = rank_pnpl_scenes(sc, _pack_quality(quality, sizes is not None, sc.device), _pack_quality(line_quality, line_sizes is not None, sc.device))

    def solve(Qh, Bh):  # the minimal solves of a fixed budget or of a round, at the cost seam
        return solve_minimal_costs(Qh, Bh, eps=eps, max_iters=max_iters, device=sc.device, **solver_opts)

    adaptive = None
    if conf is not None:
        cap = int(n_hyp)
        stage = lambda act, A, h0, Hr: solve(*sample_assemble_active(sc, act, A, h0, Hr, cap, order, pool_full or 0))  # noqa: E731
        lo_steps = None
        if local_opt:  # the rounds as without it, each ending in local_opt refits of the running bests
            state = lo_init(sc, adaptive_pnpl_init(sc))
            steps = lo_thresholds(thresh, local_opt, lo_widen)

            def lo_steps(A):
                for thresh_k in steps:
                    Bt, Qt, cnt = lo_assemble_pnpl_active(sc, state, A, thresh_k)
                    fit = solve_cost_batch(Qt, Bt, eps=eps, max_iters=max_iters, device=sc.device, **solver_opts)
                    lo_update_pnpl_active(sc, state, A, cap, conf, fit, cnt, thresh)
        else:
            state = adaptive_pnpl_init(sc)
        adaptive = (state, _rounds(sc, state, (stage, score_pnpl_active, update_pnpl_active), cap, conf, round_hyp, thresh, after_update=lo_steps), conf)
        R, t, head, mp, ml = state.R, state.t, state.head, state.mask, state.mask_lines
    else:  # no torch kernel from here to the read-back: draw + minimal assembly, the F * n_hyp minimal solves at the cost seam ...
        if order is None:
            res = solve(*sample_assemble_scenes(sc, n_hyp))
        else:  # the round sampler over the identity active list: problem f * n_hyp + h, the fixed layout
            res = solve(*sample_assemble_active(sc, torch.arange(F, dtype=torch.int32, device=sc.device), F, 0, int(n_hyp), int(n_hyp), order, pool_full))
        count = score_pnpl_scenes(sc, res.R, res.t, thresh, status=res.status, usable=(0, 2))
        R, t, head, mp, ml = select_pnpl_scenes(sc, count, res.R, res.t, res.status, thresh)
    out = _finish(sc, (assemble_pnpl_consensus, refit_update_pnpl_scenes, (("inliers_pts", "offsets"), ("inliers_lines", "line_offsets"))), R, t, head,
                  (mp, ml), thresh, refit, refit_rounds, polish, n_hyp, adaptive, pool_full)
    if local_opt:  # (the call without local optimisation keeps exactly its keys)
        out.update(lo_taken=state.lo_taken.cpu(), local_opt=local_opt, lo_widen=lo_widen)
    return out


def ransac_pnl_batch(line_2d, line_3d, K, **kw):
    """Robust PnL for F scenes of lines: ransac_pnpl_batch without points (packed lines: `line_sizes`; a guided call: `line_quality`)."""
    return ransac_pnpl_batch(None, line_2d, None, line_3d, K, **kw)


def ransac_pnpl(pts_2d, line_2d, pts_3d, line_3d, K, **kw):
    """Robust PnPL for ONE scene: pts_2d [P,2], line_2d [L,2,2], pts_3d [P,3], line_3d [L,2,3] (either pair may be None), K [3,3].  The
    batch call with F = 1 (scene 0 uses `seed` itself), unpacked: R [3,3], t [3], inliers_pts [P], inliers_lines [L] on the device;
    n_inliers, status, n_certified, best_index (ints), n_hyp.  The adaptive and guided keywords pass through (quality [P], line_quality
    [L]); hyp_used is then an int, and so is lo_taken of a call with local_opt."""
    for k in ("quality", "line_quality"):
        if kw.get(k) is not None:
            kw[k] = [kw[k]]
    out = ransac_pnpl_batch(None if pts_2d is None else [pts_2d], None if line_2d is None else [line_2d], None if pts_3d is None else [pts_3d],
                            None if line_3d is None else [line_3d], K, **kw)
    h = out["head"][0]
    one = {"R": out["R"][0], "t": out["t"][0], "inliers_pts": out["inliers_pts"], "inliers_lines": out["inliers_lines"], "n_inliers": int(h[1]),
           "status": int(h[0]), "n_certified": int(h[3]), "best_index": int(h[2]), "n_hyp": out["n_hyp"]}
    if "hyp_used" in out:
        one.update(hyp_used=int(out["hyp_used"][0]), rounds=out["rounds"], confidence=out["confidence"])
    if "pool_full" in out:
        one["pool_full"] = out["pool_full"]
    if "lo_taken" in out:
        one.update(lo_taken=int(out["lo_taken"][0]), local_opt=out["local_opt"], lo_widen=out["lo_widen"])
    return one


def ransac_pnl(line_2d, line_3d, K, **kw):
    """Robust PnL for ONE scene: ransac_pnpl without points."""
    return ransac_pnpl(None, line_2d, None, line_3d, K, **kw)
