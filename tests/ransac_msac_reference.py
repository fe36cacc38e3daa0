"""Reference of MSAC scoring, numpy only: it shares no code with the library.

gain_count: the gain and the inlier count of poses over one scene, in float64 or -- its own error bar -- np.longdouble:

    X_c = R P + t,  (u, v, w) = K X_c,  r^2 = |(u / w, v / w) - x|^2,  inlier: X_c.z > 0 and r^2 < tau^2  (a NaN compares false)
    count = number of inliers,  gain = sum over the inliers of (tau^2 - r^2) / tau^2

argmax_first: the selection -- a gain that is not > 0 reads as 0, the first of equal maxima wins.
simulate_msac: ransac_adaptive_reference.simulate's replay of the rounds with the gains deciding and the counts feeding `needed`.
perturbed_poses: host-made poses around a ground truth whose gains span 0 .. M."""
import numpy as np

from ransac_adaptive_reference import needed


def gain_count(x, X, K, R, t, thresh, dtype=np.float64):
    """x [M,2], X [M,3], K [3,3], R [H,3,3], t [H,3] -> gain [H] (dtype), count [H] int64, margin: min |r^2 - tau^2| / tau^2 over all pairs
    with a finite r^2 (inf when there is none)."""
    x, X, K, R, t = (np.asarray(a, dtype=dtype) for a in (x, X, K, R, t))
    th2 = dtype(thresh) * dtype(thresh)
    with np.errstate(all="ignore"):
        Xc = np.einsum("hij,mj->hmi", R, X) + t[:, None, :]
        uvw = np.einsum("ij,hmj->hmi", K, Xc)
        du = uvw[..., 0] / uvw[..., 2] - x[None, :, 0]
        dv = uvw[..., 1] / uvw[..., 2] - x[None, :, 1]
        r2 = du * du + dv * dv
        inl = (Xc[..., 2] > 0) & (r2 < th2)
        gain = np.where(inl, th2 - r2, dtype(0)).sum(axis=1) / th2 if th2 > 0 else np.zeros(len(R), dtype=dtype)
        fin = np.isfinite(r2)
        margin = float(np.min(np.abs(r2[fin] - th2) / th2)) if fin.any() and th2 > 0 else np.inf
    return gain, inl.sum(axis=1).astype(np.int64), margin


def gain_count_scenes(x, X, sizes, K, R, t, thresh, status=None, usable=(0, 2), dtype=np.float64):
    """Packed scenes (sizes [F]), K [3,3] or [F,3,3], hypotheses (R, t, status)[f * H + h] -> gain [F*H], count [F*H], the least margin.
    A hypothesis whose status is outside `usable` gains 0 and counts 0."""
    F, K = len(sizes), np.asarray(K)
    H = len(R) // F
    off = np.concatenate([[0], np.cumsum(sizes)])
    gain, count, margin = np.zeros(F * H, dtype=dtype), np.zeros(F * H, dtype=np.int64), np.inf
    for f in range(F):
        s, rows = slice(off[f], off[f + 1]), slice(f * H, (f + 1) * H)
        g, c, m = gain_count(x[s], X[s], K[f] if K.ndim == 3 else K, R[rows], t[rows], thresh, dtype)
        if status is not None:
            ok = np.isin(np.asarray(status)[rows], list(usable))
            g, c = np.where(ok, g, dtype(0)), np.where(ok, c, 0)
        gain[rows], count[rows], margin = g, c, min(margin, m)
    return gain, count, margin


def gain_read(gain):
    """a gain that is not > 0 (negative, NaN) reads as 0"""
    g = np.asarray(gain, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(g > 0, g, 0.0)


def argmax_first(gain):
    """index of the highest gain as read; numpy's argmax returns the first of equal maxima"""
    return int(np.argmax(gain_read(gain)))


def simulate_msac(gains, counts, status, sizes, p, round_hyp, cap):
    """gains, counts, status: [F, H] with H >= cap.  The replay of ransac_adaptive_reference.simulate with the gains deciding: returns
    hyp_used, winner, best (the COUNT of the running winner, which feeds the stopping rule), best_gain, certified [F], active (one int
    array of scene indices per round) and margins (a list of (scene, drawn, N) for every decision taken)."""
    gains, counts, status = gain_read(gains), np.asarray(counts), np.asarray(status)
    F = gains.shape[0]
    assert gains.shape[1] >= cap and counts.shape == gains.shape == status.shape and len(sizes) == F
    hyp_used, winner, certified = (np.zeros(F, dtype=np.int64) for _ in range(3))
    best, best_gain = np.full(F, -1, dtype=np.int64), np.full(F, -1.0)
    active, rounds, margins, h0 = np.arange(F), [], [], 0
    while len(active) and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        rounds.append(active.copy())
        keep = []
        for f in active:
            g = gains[f, h0:h0 + Hr]
            j = int(np.argmax(g))
            if g[j] > best_gain[f]:            # strictly greater: an earlier round keeps a tie
                best_gain[f], best[f], winner[f] = g[j], counts[f, h0 + j], h0 + j
            certified[f] += int((status[f, h0:h0 + Hr] == 0).sum())
            drawn = h0 + Hr
            hyp_used[f] = drawn
            N = needed(best[f], sizes[f], p)
            margins.append((int(f), drawn, N))
            if not (drawn >= N or drawn >= cap):
                keep.append(f)
        active = np.array(keep, dtype=np.int64)
        h0 += Hr
    return {"hyp_used": hyp_used, "winner": winner, "best": best, "best_gain": best_gain, "certified": certified, "active": rounds,
            "margins": margins}


def _rodrigues(w):
    a = np.linalg.norm(w)
    if a == 0:
        return np.eye(3)
    k = w / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def perturbed_poses(R_gt, t_gt, H, rs, max_deg=2.0, max_rel=0.05):
    """H poses around (R_gt, t_gt): rotations by 0 .. max_deg degrees about random axes, translations off by 0 .. max_rel of |t_gt|, both
    growing with h (each between half and all of its share h / (H - 1)) -- pose 0 is the ground truth, so that the gains span 0 .. M."""
    R, t = np.zeros((H, 3, 3)), np.zeros((H, 3))
    for h in range(H):
        s = h / max(H - 1, 1)
        axis = rs.normal(size=3)
        axis /= np.linalg.norm(axis)
        R[h] = _rodrigues(axis * np.deg2rad(max_deg) * s * (0.5 + 0.5 * rs.random_sample())) @ R_gt
        d = rs.normal(size=3)
        t[h] = t_gt + d / np.linalg.norm(d) * np.linalg.norm(t_gt) * max_rel * s * (0.5 + 0.5 * rs.random_sample())
    return R, t


def rotation_error_deg(R, R_gt):
    c = 0.5 * (np.trace(np.asarray(R).T @ np.asarray(R_gt)) - 1.0)
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
