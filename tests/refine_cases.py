"""What the refinement tests share: the synthetic problems, their starts, the edge-case batch and the checks against
tests/refine_reference.py.  The bars are those of the issue that introduced the library: the reference's next step from a returned pose
is at most 1e-6 (the project's parity bar against its oracle), and the covariance agrees with the reference's normal equations to
1e3 cond(J^T J) eps, derived per problem."""
import numpy as np

import refine_reference as ref
from cvxpnpl_amd import synth

EPS = np.finfo(np.float64).eps
STEP_BAR = 1e-6
SHAPES = ((10, 0, 1.0), (5, 5, 1.0), (17, 0, 2.0), (33, 7, 1.0), (0, 6, 1.0), (4, 0, 1.0))  # the six over-determined shapes (n_p, n_l, sigma)


def problem(batch, n_p, n_l, sigma, seed=11, rot=0.05, rel_t=0.05):
    """synth.make_pnpl started `rot` rad and `rel_t` of t off the truth; returns (data dict, R0, t0, kw) with kw the correspondence
    arguments of refine_pose_batch(_host)."""
    d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=seed)
    rs = np.random.RandomState(seed + 1)
    ax = rs.normal(size=(batch, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    R0 = np.stack([ref.expm_so3(rot * a) @ R for a, R in zip(ax, d["R_gt"])])
    t0 = d["t_gt"] * (1.0 + rel_t * rs.uniform(-1.0, 1.0, size=(batch, 3)))
    kw = {"pts_2d": d["pts_2d"] if n_p else None, "pts_3d": d["pts_3d"] if n_p else None,
          "line_2d": d["line_2d"] if n_l else None, "line_3d": d["line_3d"] if n_l else None}
    return d, R0, t0, kw


def one(kw, b, **extra):
    """Problem b of a batch, as the keyword arguments of the reference."""
    out = {k: v[b] for k, v in kw.items() if v is not None}
    out.update(extra)
    return out


def worst_next_step(K, R, t, kw, rows=None, masks=None):
    """max over the problems of |step| the REFERENCE would take next from (R[b], t[b]) at lambda_0."""
    worst = 0.0
    for b in (range(len(R)) if rows is None else rows):
        extra = {} if masks is None else {k: v[b] for k, v in masks.items() if v is not None}
        Kb = K[b] if np.ndim(K) == 3 else K
        d, _, _ = ref.lm_step(Kb, R[b], t[b], **one(kw, b, **extra))
        worst = max(worst, float(np.linalg.norm(d)))
    return worst


def worst_cov_ratio(K, out, kw, sigma_px=0.0, rows=None):
    """max over the problems of |cov (J^T J_ref / sigma^2) - I|_max / (1e3 cond(J^T J_ref) eps): at most 1 when the bound holds."""
    worst = 0.0
    for b in (range(len(out.R)) if rows is None else rows):
        Kb = K[b] if np.ndim(K) == 3 else K
        _, A, r = ref.lm_step(Kb, out.R[b], out.t[b], **one(kw, b))
        s2 = sigma_px**2 if sigma_px > 0 else out.cost[b, 1] / (len(r) - 6)
        E = out.cov[b] @ (A / s2) - np.eye(6)
        worst = max(worst, float(np.abs(E).max() / (1e3 * np.linalg.cond(A) * EPS)))
    return worst


def edge_batch():
    """One batch of (8 points, 4 lines) problems holding every pass-through case beside live ones.  Returns (K, R0, t0, kw, status_in,
    masks, expected status per problem)."""
    B = 12
    d, R0, t0, kw = problem(B, 8, 4, 1.0, seed=23)
    kw = {k: v.copy() for k, v in kw.items()}
    status_in = np.zeros(B, np.int32)
    mp, ml = np.ones((B, 8), np.uint8), np.ones((B, 4), np.uint8)
    expect = np.zeros(B, np.int32)
    R0[1, 0, 0] = np.nan                                         # a NaN pose
    expect[1] = 2
    R0[2, 1] = -R0[2, 1]                                         # a reflection
    expect[2] = 2
    status_in[3] = 1                                             # a status outside admit_mask (0x5)
    expect[3] = 2
    status_in[4] = 2                                             # ... and one inside it beside status 0
    mp[5, 2:] = 0                                                # 2 live correspondences
    ml[5] = 0
    expect[5] = 3
    Y = kw["pts_3d"][6, 0] @ R0[6].T                             # one live point behind the camera
    t0[6, 2] = -Y[2] - 0.1
    expect[6] = 4
    kw["line_2d"][7, 1, 1] = kw["line_2d"][7, 1, 0]              # a degenerate 2D line among good ones: not live, the rest refine
    t0[8] = np.inf                                               # a non-finite translation
    expect[8] = 2
    return d["K"], R0, t0, kw, status_in, {"mask_pts": mp, "mask_lines": ml}, expect


def check_edge_batch(out, R0, t0, expect):
    assert out.status.tolist() == expect.tolist(), (out.status, expect)
    for b in np.nonzero(expect >= 2)[0]:
        assert out.R[b].tobytes() == R0[b].tobytes() and out.t[b].tobytes() == t0[b].tobytes(), b   # bit for bit
        assert np.isnan(out.cost[b]).all() and out.iters[b] == 0, b
        if out.cov is not None:
            assert np.isnan(out.cov[b]).all(), b
    live = np.nonzero(expect < 2)[0]
    assert np.isfinite(out.R[live]).all() and np.isfinite(out.cost[live]).all()
    assert (out.cost[live, 1] <= out.cost[live, 0]).all()
    n_live = np.full(len(expect), 12)
    n_live[5], n_live[7] = 2, 11
    assert out.n_live.tolist() == n_live.tolist(), out.n_live
