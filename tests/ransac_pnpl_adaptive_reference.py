"""Reference of adaptive and guided RANSAC over points and lines, numpy only: it shares no code with the library.

A scene's correspondences are indexed over the UNION of its P points and L lines: c < P is point c, otherwise line c - P.  The two rules
know nothing of what a correspondence is, so the restatements are those of the point versions on M = P + L:
union_rank(quality, line_quality): the ranking of the union, best first (ransac_guided_reference.rank on points-then-lines).
guided_union_sets(H, P, L, order, pool_full, seed, h0): the minimal sets order[pick] of hypotheses h0 .. h0 + H - 1.
replay(counts, status, shapes, p, round_hyp, cap): the rounds on GIVEN counts (ransac_adaptive_reference.simulate on M_f = P_f + L_f).
packed_order(orders, shapes): the per-scene rankings laid out as the library packs them, scene f from off_p[f] + off_l[f] on."""
import numpy as np

from ransac_adaptive_reference import simulate
from ransac_guided_reference import guided_sets, rank


def union_rank(quality, line_quality):
    qp = np.zeros(0) if quality is None else np.asarray(quality, dtype=np.float64).reshape(-1)
    ql = np.zeros(0) if line_quality is None else np.asarray(line_quality, dtype=np.float64).reshape(-1)
    return rank(np.concatenate([qp, ql]))


def guided_union_sets(H, P, L, order, pool_full, seed, h0=0):
    """idx [H, 4] of union indices; order: a permutation of 0 .. P + L - 1, best first."""
    return guided_sets(H, int(P) + int(L), order, pool_full, seed, h0=h0)


def replay(counts, status, shapes, p, round_hyp, cap):
    return simulate(counts, status, [int(a) + int(b) for a, b in shapes], p, round_hyp, cap)


def packed_order(orders, shapes):
    """int32 [sum P + sum L]: scene f's ranking at beg_f = sum_{g < f} (P_g + L_g) = off_p[f] + off_l[f]."""
    assert len(orders) == len(shapes) and all(len(o) == p + l for o, (p, l) in zip(orders, shapes))
    return np.concatenate([np.asarray(o, dtype=np.int32) for o in orders]) if orders else np.zeros(0, np.int32)
