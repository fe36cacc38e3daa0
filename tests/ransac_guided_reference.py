"""Reference of guided RANSAC's sampler, numpy only: it shares no code with the library.

pool(h, M, pool_full): the number of best-ranked correspondences hypothesis h draws from (linear search); pools(hs, ...) the same for an
array of h.  rank(quality): the ranking, best first.  guided_sets(H, M, order, pool_full, seed): the minimal sets of one scene, built from
synth.philox_minimal_sets per distinct pool size.  quality_patterns / planted_quality: the inputs the CPU and GPU tests share."""
import numpy as np


def _growth(M, pool_full):
    """T(n) for n = 4 .. M: pool_full * ((n/M) * ((n-1)/(M-1)) * ((n-2)/(M-2)) * ((n-3)/(M-3))), float64, in this order."""
    n, Md = np.arange(4, int(M) + 1, dtype=np.float64), np.float64(M)
    return np.float64(pool_full) * ((n / Md) * ((n - 1.0) / (Md - 1.0)) * ((n - 2.0) / (Md - 2.0)) * ((n - 3.0) / (Md - 3.0)))


def pool(h, M, pool_full):
    h, M, pool_full = int(h), int(M), int(pool_full)
    assert h >= 0 and M >= 4 and pool_full >= 0
    if h >= pool_full:
        return M
    ok = np.nonzero(_growth(M, pool_full) >= np.float64(h + 1))[0]   # linear: the first n that reaches h + 1
    n_T = 4 + int(ok[0]) if len(ok) else M
    return min(n_T, 4 + h, M)


def pools(hs, M, pool_full):
    """pool() for an int64 array of hypothesis indices.  T is non-decreasing, so the first n reaching h + 1 is a sorted search."""
    hs, M, pool_full = np.asarray(hs, dtype=np.int64), int(M), int(pool_full)
    T = _growth(M, pool_full)
    assert (np.diff(T) >= 0).all()
    j = np.searchsorted(T, (hs + 1).astype(np.float64), side="left")
    n_T = np.where(j < len(T), 4 + j, M)
    return np.where(hs >= pool_full, M, np.minimum(np.minimum(n_T, 4 + hs), M)).astype(np.int64)


def rank(quality):
    """Indices best first: quality descending, equal qualities by index; a NaN counts as -inf."""
    q = np.asarray(quality, dtype=np.float64)
    key = np.where(np.isnan(q), -np.inf, q)
    return np.argsort(-key, kind="stable").astype(np.int64)


def guided_sets(H, M, order, pool_full, seed, h0=0):
    """idx [H, 4]: the minimal sets of hypotheses h0 .. h0 + H - 1 of a scene of M correspondences ranked by `order`."""
    from cvxpnpl_amd import synth

    order = np.asarray(order, dtype=np.int64)
    hs = np.arange(h0 + H, dtype=np.int64)
    n = pools(hs, M, pool_full)
    idx = np.zeros((h0 + H, 4), dtype=np.int64)
    for size in np.unique(n):
        rows = np.nonzero(n == size)[0]
        idx[rows] = synth.philox_minimal_sets(int(rows.max()) + 1, int(size), 4, int(seed))[rows]
    before = hs < pool_full
    idx[before] = order[idx[before]]   # ranks to scene indices; from pool_full on the draw is the scene index itself
    return idx[h0:]


def first_all_inlier(sets, inlier):
    """Index of the first minimal set whose four correspondences are all inliers, or -1."""
    hit = np.nonzero(np.asarray(inlier, dtype=bool)[sets].all(axis=1))[0]
    return int(hit[0]) if len(hit) else -1


def planted_quality(inlier, rs):
    """A matcher's score that knows something: U(0.2, 1) on the inliers, U(0, 0.8) on the clutter."""
    inlier = np.asarray(inlier, dtype=bool)
    return np.where(inlier, rs.uniform(0.2, 1.0, len(inlier)), rs.uniform(0.0, 0.8, len(inlier)))


def quality_patterns(M, rs):
    """The qualities the ranking is tested on, by name."""
    special = rs.random_sample(M)
    for j, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 0.0, -np.inf, np.inf)):
        special[(j * 7) % M] = v
    return {"random": rs.random_sample(M), "all_equal": np.full(M, 0.25), "duplicates": rs.randint(0, 3, M).astype(np.float64),
            "ascending": np.arange(M, dtype=np.float64), "descending": -np.arange(M, dtype=np.float64), "special": special}
