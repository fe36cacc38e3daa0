"""Reference of adaptive RANSAC's bookkeeping, numpy only: it shares no code with the library.

needed(I, M, p): the standard stopping rule for minimal sets of four drawn without replacement.
simulate(counts, status, sizes, p, round_hyp, cap): replays the rounds on GIVEN counts and says, per scene, after how many hypotheses it
stops, which hypothesis wins, how many certified hypotheses it saw, and which scenes are active in every round."""
import numpy as np


def needed(I, M, p):
    """N = log(1 - p) / log(1 - q), q = I (I-1) (I-2) (I-3) / (M (M-1) (M-2) (M-3)); inf when I < 4, 0 when I >= M."""
    I, M = int(I), int(M)
    if I < 4 or M < 4:
        return np.inf
    if I >= M:
        return 0.0
    q = np.float64(1.0)
    for j in range(4):
        q = q * (np.float64(I - j) / np.float64(M - j))
    return float(np.log(np.float64(1.0) - np.float64(p)) / np.log1p(-q))


def simulate(counts, status, sizes, p, round_hyp, cap):
    """counts, status: [F, H] with H >= cap (hypothesis h of scene f); sizes [F].  Returns a dict:
    hyp_used [F], winner [F] (index within the scene; the lowest index among the highest counts of the first hyp_used[f] hypotheses),
    best [F] (its count), certified [F] (status == 0 among them), active (a list, one int array of scene indices per round, in order),
    margins (a list of (scene, round, drawn, N) for every decision taken)."""
    counts, status = np.asarray(counts), np.asarray(status)
    F = counts.shape[0]
    assert counts.shape[1] >= cap and status.shape == counts.shape and len(sizes) == F
    hyp_used = np.zeros(F, dtype=np.int64)
    winner = np.zeros(F, dtype=np.int64)
    best = np.full(F, -1, dtype=np.int64)
    certified = np.zeros(F, dtype=np.int64)
    active, rounds, margins = np.arange(F), [], []
    h0, r = 0, 0
    while len(active) and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        rounds.append(active.copy())
        keep = []
        for f in active:
            c = counts[f, h0:h0 + Hr]
            j = int(np.argmax(c))              # numpy's argmax returns the first of equal maxima
            if c[j] > best[f]:                 # strictly greater: an earlier round keeps a tie
                best[f], winner[f] = c[j], h0 + j
            certified[f] += int((status[f, h0:h0 + Hr] == 0).sum())
            drawn = h0 + Hr
            hyp_used[f] = drawn
            N = needed(best[f], sizes[f], p)
            margins.append((int(f), r, drawn, N))
            if not (drawn >= N or drawn >= cap):
                keep.append(f)
        active = np.array(keep, dtype=np.int64)
        h0 += Hr
        r += 1
    return {"hyp_used": hyp_used, "winner": winner, "best": best, "certified": certified, "active": rounds, "margins": margins}
