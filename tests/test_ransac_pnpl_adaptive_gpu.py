"""Adaptive and guided RANSAC over points and lines (ransac_pnpl_batch(confidence=..., quality=..., line_quality=...),
libcvxpnpl_amd_ransac_pnpl_adaptive.so).

Every stage is held against the fourth library's kernel on the same inputs (sample_assemble_scenes, score_pnpl_scenes, select_pnpl_scenes:
the fixed-budget path, whose kernels this feature leaves as they were), the guided draw and the bookkeeping against the numpy restatements
of tests/ransac_pnpl_adaptive_reference.py, the guided costs against assemble_batch on the gathered sets; then the whole call against
fixed-budget calls at the budgets it stopped at, against itself, and on point-only scenes against ransac_pnp_batch.  16 scenes: every
minimal mix, 5 correspondences of one kind, sizes around the wave width, one P_f above a point tile of the scoring kernel (512), one L_f
above a line tile (256); clutter 0 .. 0.6, sigma 0.5 px; once with a shared K and once with a K per scene."""
import ctypes as C

import numpy as np
import pytest

from ransac_pnpl_adaptive_reference import guided_union_sets, packed_order, replay, union_rank

pytestmark = pytest.mark.gpu

SHAPES = [(4, 0), (0, 4), (3, 1), (1, 3), (2, 2), (5, 0), (0, 5), (63, 1), (40, 25), (70, 0), (0, 70), (513, 3), (3, 257), (300, 300), (100, 50), (20, 20)]
CLUTTER = [0.0, 0.0, 0.0, 0.34, 0.0, 0.2, 0.2, 0.5, 0.3, 0.55, 0.6, 0.4, 0.5, 0.6, 0.45, 0.2]
# (0.34 of (1, 3): one displaced line, so that no hypothesis of that scene reaches four inliers and it runs to every cap)
MS = [p + l for p, l in SHAPES]
F, THRESH, SEED, CONF = len(SHAPES), 2.0, 2000, 0.99
CFG = {"rounds_of_64": (64, 200), "two_workgroups": (300, 600)}   # (round_hyp, cap); 300 = one full workgroup in x and a partial one
H_ALL = 600   # hypotheses solved once per scene: both caps are prefixes of them
POOL_FULL = 100   # inside the round 64 .. 127: a guided round that crosses h = pool_full
LISTS = {"identity": list(range(F)), "every_other": list(range(0, F, 2)), "one": [F - 3], "reversed": list(range(F - 1, -1, -1))}
assert F == 16 and len(CLUTTER) == F


def _make_scenes(per_scene_K, shapes=SHAPES, clutter=CLUTTER, seed0=300, sigma=0.5):
    from cvxpnpl_amd import synth

    out, Ks, n = [], [], len(shapes)
    for f, (p, l) in enumerate(shapes):
        K = np.array(synth.K_KINECT)
        if per_scene_K:
            K[0, 0] *= 0.8 + 0.4 * f / max(n - 1, 1)
            K[1, 1] *= 0.8 + 0.4 * f / max(n - 1, 1)
        out.append(synth.make_ransac_pnpl(p, l, outlier_frac=clutter[f], sigma=sigma, seed=seed0 + f, K=K))
        Ks.append(K)
    return out, (np.stack(Ks) if per_scene_K else Ks[0])


def _lists(scenes):
    return [d["pts_2d"] for d in scenes], [d["line_2d"] for d in scenes], [d["pts_3d"] for d in scenes], [d["line_3d"] for d in scenes]


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One frame set per K mode, computed once: scenes, H_ALL minimal sets per scene by the fourth library's sampler, their solves and
    counts; a quality per correspondence and the ranking of every scene's union.  Nothing below changes it."""
    import torch

    from cvxpnpl_amd import _lib, ransac as rn
    from ransac_guided_reference import planted_quality

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_pnpl_lib(); _lib.ransac_adaptive_lib(); _lib.ransac_guided_lib(); _lib.ransac_pnpl_adaptive_lib()
    s = _State()
    s.dev = torch.device("cuda:0")
    s.per = request.param == "per_scene_K"
    s.scenes, s.K = _make_scenes(s.per)
    s.args = _lists(s.scenes)
    s.Kf = [s.K[f] if s.per else s.K for f in range(F)]
    s.seeds = [SEED + f for f in range(F)]
    s.sc = rn.pack_pnpl_scenes(*s.args, s.K, device=s.dev, seeds=s.seeds)
    s.offp = np.concatenate([[0], np.cumsum([p for p, _ in SHAPES])])
    s.offl = np.concatenate([[0], np.cumsum([l for _, l in SHAPES])])
    s.offu = s.offp + s.offl
    s.Q, s.B, s.idx = rn.sample_assemble_scenes(s.sc, H_ALL, want_idx=True)
    s.res = rn.solve_minimal_costs(s.Q, s.B, eps=1e-6, max_iters=100)   # (as ransac_pnpl_batch solves them)
    s.count = rn.score_pnpl_scenes(s.sc, s.res.R, s.res.t, THRESH, status=s.res.status, usable=(0, 2))
    rs = np.random.RandomState(17)
    s.qp = [planted_quality(d["inlier_pts"], rs) for d in s.scenes]
    s.ql = [planted_quality(d["inlier_lines"], rs) for d in s.scenes]
    s.order_ref = [union_rank(a, b) for a, b in zip(s.qp, s.ql)]
    s.order = rn.rank_pnpl_scenes(s.sc, torch.as_tensor(np.concatenate(s.qp)).to(s.dev), torch.as_tensor(np.concatenate(s.ql)).to(s.dev))
    torch.cuda.synchronize()
    s.count_h = s.count.cpu().numpy().reshape(F, H_ALL)
    s.status_h = s.res.status.cpu().numpy().reshape(F, H_ALL)
    return s


def _rows(full, n_scenes, act, h0, Hr):
    """rows [f, h0 : h0 + Hr] for f in act of a tensor laid out [n_scenes * H, ...], as one contiguous [len(act) * Hr, ...] tensor"""
    import torch

    H = full.shape[0] // n_scenes
    v = full.reshape((n_scenes, H) + tuple(full.shape[1:]))
    a = torch.as_tensor(np.asarray(act, dtype=np.int64), device=full.device)
    return v[a, h0:h0 + Hr].reshape((len(act) * Hr,) + tuple(full.shape[1:])).contiguous()


def _bits(a, b):
    """equal bit for bit: float64 as words, so that a NaN equals itself and +0 differs from -0"""
    import torch

    return torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _margins_hold(sim):
    """The condition under which a last-bit difference between the device's and numpy's log cannot flip a decision."""
    for f, r, drawn, N in sim["margins"]:
        if np.isfinite(N):
            assert abs(drawn - N) > 1e-6 * max(N, 1.0), f"scene {f} round {r}: drawn {drawn} against N {N}: change the seed"


# ---- 0. what the inputs exercise, from the reference alone ---------------------------------------------------------------------------------
def test_the_reference_sees_every_path(st):
    import torch

    rh, cap = CFG["rounds_of_64"]
    sim = replay(st.count_h, st.status_h, SHAPES, CONF, rh, cap)
    _margins_hold(sim)
    used = sim["hyp_used"]
    print("hyp_used", list(used), "best", list(sim["best"]), "active per round", [len(a) for a in sim["active"]])
    assert (used == 64).any() and ((used == 128) | (used == 192)).any() and (used == cap).any()   # stops in different rounds, and the cap
    assert len(sim["active"]) == 4 and cap - 3 * rh == 8                                          # the last round is short: Hr = 8
    rh2, cap2 = CFG["two_workgroups"]
    sim2 = replay(st.count_h, st.status_h, SHAPES, CONF, rh2, cap2)
    _margins_hold(sim2)
    assert len(sim2["active"]) == 2 and (sim2["hyp_used"] == 300).any() and (sim2["hyp_used"] == 600).any()
    # the ranking of the unions: cvxpnpl_ransac_guided_rank over the union offsets equals the numpy ranking
    assert np.array_equal(st.order.cpu().numpy(), packed_order(st.order_ref, SHAPES))
    assert st.order.dtype == torch.int32 and st.order.shape == (st.offu[-1],)


# ---- 1. the round sampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h0", [0, 64, 192])
def test_sampler_equals_the_rows_of_the_fixed_sampler_bit_for_bit(st, h0):
    import torch

    from cvxpnpl_amd import ransac as rn

    for rh, cap in CFG.values():
        if h0 >= cap:
            continue
        Hr = min(rh, cap - h0)
        for name, act in LISTS.items():
            a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
            for kw in ({}, {"order": st.order, "pool_full": 0}):   # a ranking that pool_full = 0 never reads
                Q, B, idx = rn.sample_assemble_active(st.sc, a, len(act), h0, Hr, cap, want_idx=True, **kw)
                assert idx.shape == (len(act) * Hr, 4) and Q.shape == (len(act) * Hr, 45) and B.shape == (len(act) * Hr, 27)
                assert torch.equal(idx, _rows(st.idx, F, act, h0, Hr)), (name, rh, kw.keys())
                assert _bits(Q, _rows(st.Q, F, act, h0, Hr)) and _bits(B, _rows(st.B, F, act, h0, Hr)), (name, rh, kw.keys())   # NaN patterns included
    # a longer tensor than n_active: only the first n_active entries count
    a = torch.as_tensor(list(range(F)), dtype=torch.int32, device=st.dev)
    Q, _ = rn.sample_assemble_active(st.sc, a, 3, h0, 8, 200)
    assert _bits(Q, _rows(st.Q, F, [0, 1, 2], h0, 8))


def test_what_the_sampler_cannot_assemble_equals_the_fixed_sampler_too(st):
    """A scene forced below four correspondences through the stage function, and a singular K: NaN cost and idx = -1, as the rows of
    sample_assemble_scenes on the same scene set."""
    import torch

    from cvxpnpl_amd import ransac as rn

    sc, j = st.sc, 8
    Ks = sc.K.clone()
    if st.per:
        Ks[j, 2, 2] = 0.0
    else:
        Ks[2, 2] = 0.0
    sing = rn.PnplScenes(sc.x, sc.X, sc.l2, sc.l3, sc.offsets, sc.line_offsets, sc.sizes, sc.line_sizes, Ks, sc.seeds)
    loff = sc.line_offsets.clone()
    loff[3] = loff[2]   # scene 2, (3, 1), hands its line to scene 3: three correspondences are left to it
    short = rn.PnplScenes(sc.x, sc.X, sc.l2, sc.l3, sc.offsets, loff, sc.sizes, sc.line_sizes, sc.K, sc.seeds)
    a = torch.arange(F, dtype=torch.int32, device=st.dev)
    for cut, f in ((sing, j), (short, 2)):
        Q0, B0, i0 = rn.sample_assemble_scenes(cut, 64, want_idx=True)
        Q, B, idx = rn.sample_assemble_active(cut, a, F, 0, 64, 64, st.order, 0, want_idx=True)
        assert torch.isnan(Q[f * 64:(f + 1) * 64]).all() and (idx[f * 64:(f + 1) * 64] == -1).all()
        assert _bits(Q, Q0) and _bits(B, B0) and torch.equal(idx, i0)


def _gathered(scene, P, idx):
    """the sets idx [n, 4] (union indices) of one scene, grouped by shape: {k_p: (rows, p2 [n,k_p,2], l2 [n,k_l,2,2], p3, l3)}, each set
    ordered points in draw order, then lines in draw order"""
    srt = np.take_along_axis(idx, np.argsort(idx >= P, axis=1, kind="stable"), 1)
    kp = (idx < P).sum(1)
    out = {}
    for k in np.unique(kp):
        rows = np.nonzero(kp == k)[0]
        ip, il = srt[rows][:, :k], srt[rows][:, k:] - P
        out[int(k)] = (rows, scene["pts_2d"][ip], scene["line_2d"][il], scene["pts_3d"][ip], scene["line_3d"][il])
    return out


@pytest.mark.parametrize("h0", [0, 64])
def test_guided_sampler_equals_the_numpy_draw_and_assemble_batch(st, h0):
    """idx exactly, also across h = pool_full (inside the round of h0 = 64); Q45 and B27 within the bounds of tests/test_ransac_pnpl_gpu.py
    against assemble_batch on the gathered sets: |dQ| <= 1e-11 max|Q|, |dB| <= 1e-9 max(1, max|B|) per set."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    Hr, cap = 64, 200
    assert h0 <= POOL_FULL < h0 + Hr or h0 + Hr <= POOL_FULL
    for name in ("identity", "reversed", "one"):
        act = LISTS[name]
        a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
        Q, B, idx = rn.sample_assemble_active(st.sc, a, len(act), h0, Hr, cap, st.order, POOL_FULL, want_idx=True)
        ref = np.concatenate([guided_union_sets(Hr, *SHAPES[f], st.order_ref[f], POOL_FULL, st.seeds[f], h0=h0) for f in act])
        assert np.array_equal(idx.cpu().numpy(), ref), name
        if name != "identity":
            continue
        Qn, Bn = Q.cpu().numpy(), B.cpu().numpy()
        worst_q = worst_b = 0.0
        for i, f in enumerate(act):
            for k, (rows, p2, l2, p3, l3) in _gathered(st.scenes[f], SHAPES[f][0], ref[i * Hr:(i + 1) * Hr]).items():
                g = i * Hr + rows
                Bs, Qs = ca.assemble_batch(p2 if k else None, l2 if k < 4 else None, p3 if k else None, l3 if k < 4 else None, st.Kf[f], device=st.dev,
                                           blocked=False)
                Bs, Qs = Bs.cpu().numpy(), Qs.cpu().numpy()
                fin = np.isfinite(Qs).all(1)
                assert np.array_equal(np.isfinite(Qn[g]).all(1), fin) and np.array_equal(np.isfinite(Bn[g]).all(1), fin), (f, k)
                eq = np.abs(Qn[g] - Qs).max(1) / np.abs(Qs).max(1)
                eb = np.abs(Bn[g] - Bs).max(1) / np.maximum(1.0, np.abs(Bs).max(1))
                worst_q, worst_b = max(worst_q, float(eq[fin].max(initial=0))), max(worst_b, float(eb[fin].max(initial=0)))
        print(f"guided minimal assembly, h0 = {h0}: max |dQ| / max|Q| = {worst_q:.3e}, max |dB| / max(1, |B|) = {worst_b:.3e} against assemble_batch")
        assert worst_q <= 1e-11 and worst_b <= 1e-9, (worst_q, worst_b)


def test_an_order_entry_out_of_range_is_never_followed(st):
    """One entry of one scene's ranking outside [0, M_f): NaN and idx = -1 for the hypotheses that read it, and for nothing else."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth
    from ransac_guided_reference import pools

    f, r, Hr, cap = 8, 2, 128, 200   # scene (40, 25), the third-best rank
    a = torch.arange(F, dtype=torch.int32, device=st.dev)
    Q0, B0, i0 = rn.sample_assemble_active(st.sc, a, F, 0, Hr, cap, st.order, POOL_FULL, want_idx=True)
    hs = np.arange(Hr)
    n = pools(hs, MS[f], POOL_FULL)
    ranks = np.zeros((Hr, 4), dtype=np.int64)
    for size in np.unique(n):
        rows = np.nonzero(n == size)[0]
        ranks[rows] = synth.philox_minimal_sets(int(rows.max()) + 1, int(size), 4, st.seeds[f])[rows]
    reads = (ranks == r).any(1) & (hs < POOL_FULL)
    assert reads.any() and not reads.all() and reads[0]   # (hypothesis 0 draws the four best ranks)
    for badv in (MS[f], -1, 2**31 - 1):
        order = st.order.clone()
        order[st.offu[f] + r] = badv
        Q, B, idx = rn.sample_assemble_active(st.sc, a, F, 0, Hr, cap, order, POOL_FULL, want_idx=True)
        hit = torch.zeros(F * Hr, dtype=torch.bool, device=st.dev)
        hit[f * Hr:(f + 1) * Hr] = torch.as_tensor(reads, device=st.dev)
        assert torch.isnan(Q[hit]).all() and torch.isnan(B[hit]).all() and (idx[hit] == -1).all(), badv
        assert _bits(Q[~hit], Q0[~hit]) and _bits(B[~hit], B0[~hit]) and torch.equal(idx[~hit], i0[~hit]), badv


# ---- 2. scoring -----------------------------------------------------------------------------------------------------------------------------
def test_scoring_equals_the_rows_of_the_fixed_scoring(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    differing = 0
    for act in LISTS.values():
        a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
        for h0, Hr in ((0, 64), (192, 8), (0, 300), (300, 300)):
            R, t, s = (_rows(v, F, act, h0, Hr) for v in (st.res.R, st.res.t, st.res.status))
            mine = rn.score_pnpl_active(st.sc, a, len(act), R, t, THRESH, status=s, usable=(0, 2))
            differing += int((mine != _rows(st.count, F, act, h0, Hr)).sum())
    assert differing == 0, differing   # the same predicates on the same poses


# ---- 3. update and compaction ---------------------------------------------------------------------------------------------------------------
def _drive(st, count, rh, cap, status=None):
    """The rounds on given counts [F * H_ALL] (device int32): update + compact per round, the active list held against the replay at every
    round.  Returns (state, replay)."""
    import torch

    from cvxpnpl_amd import ransac as rn

    status = st.res.status if status is None else status
    sim = replay(count.cpu().numpy().reshape(F, H_ALL), status.cpu().numpy().reshape(F, H_ALL), SHAPES, CONF, rh, cap)
    _margins_hold(sim)
    state = rn.adaptive_pnpl_init(st.sc)
    assert torch.equal(state.head.cpu(), torch.tensor([[3, -1, 0, 0]] * F, dtype=torch.int32)) and int(state.n_active.cpu()) == F
    assert not state.hyp_used.any() and (state.best == -1).all()
    assert state.mask.shape == (st.offp[-1],) and state.mask_lines.shape == (st.offl[-1],)
    A, h0 = F, 0
    for r, act in enumerate(sim["active"]):
        assert A == len(act), (r, A, list(act))
        assert np.array_equal(state.active[:A].cpu().numpy(), act), (r, list(act))
        Hr = min(rh, cap - h0)
        R, t, s, c = (_rows(v, F, act, h0, Hr) for v in (st.res.R, st.res.t, status, count))
        rn.update_pnpl_active(st.sc, state, A, h0, cap, CONF, c, R, t, s, THRESH)
        rn.compact_active(st.sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
        h0 += Hr
    assert A == 0, A
    return state, sim


def _equals_the_fixed_selection(st, state, count, sim, status=None):
    """hyp_used against the replay; pose, head and both masks bit for bit against select_pnpl_scenes over each scene's first hyp_used
    hypotheses."""
    import torch

    from cvxpnpl_amd import ransac as rn

    status = st.res.status if status is None else status
    used = state.hyp_used.cpu().numpy()
    assert np.array_equal(used, sim["hyp_used"]), (list(used), list(sim["hyp_used"]))
    head = state.head.cpu().numpy()
    assert np.array_equal(head[:, 2], sim["winner"]) and np.array_equal(head[:, 3], sim["certified"])
    assert np.array_equal(state.best.cpu().numpy(), sim["best"])
    for u in sorted(set(used.tolist())):
        R, t, s, c = (_rows(v, F, range(F), 0, u) for v in (st.res.R, st.res.t, status, count))
        R1, t1, h1, mp1, ml1 = rn.select_pnpl_scenes(st.sc, c, R, t, s, THRESH)
        for f in np.nonzero(used == u)[0]:
            assert torch.equal(state.head[f], h1[f]), (f, u, state.head[f].tolist(), h1[f].tolist())
            assert _bits(state.R[f], R1[f]) and _bits(state.t[f], t1[f]), (f, u)
            assert torch.equal(state.mask[st.offp[f]:st.offp[f + 1]], mp1[st.offp[f]:st.offp[f + 1]]), (f, u)
            assert torch.equal(state.mask_lines[st.offl[f]:st.offl[f + 1]], ml1[st.offl[f]:st.offl[f + 1]]), (f, u)


@pytest.mark.parametrize("cfg", list(CFG))
def test_rounds_equal_the_fixed_selection_over_the_hypotheses_used(st, cfg):
    rh, cap = CFG[cfg]
    state, sim = _drive(st, st.count, rh, cap)
    _equals_the_fixed_selection(st, state, st.count, sim)


def test_ties_never_move_the_winner(st):
    import torch

    rh, cap = CFG["rounds_of_64"]
    flat = torch.full_like(st.count, 3)   # all counts equal (3 < 4: every scene runs to the cap): index 0 of round 0 wins and stays
    state, sim = _drive(st, flat, rh, cap)
    assert (state.head[:, 2] == 0).all() and (state.hyp_used == cap).all()
    _equals_the_fixed_selection(st, state, flat, sim)
    # a later round that only ties: hypothesis 5 of round 0 against hypothesis 70 of round 1
    c = torch.zeros_like(st.count).reshape(F, H_ALL)
    c[:, 5] = 4
    c[:, 70] = 4
    c[:, 199] = 4
    c = c.reshape(-1).contiguous()
    state, sim = _drive(st, c, rh, cap)
    assert (state.head[:, 2] == 5).all(), state.head[:, 2].tolist()
    assert int(state.hyp_used.min()) == 64 and int(state.hyp_used.max()) == cap   # (4 of 4 stops at once, 4 of 600 never)
    _equals_the_fixed_selection(st, state, c, sim)


def test_a_scene_without_a_usable_hypothesis_runs_to_the_cap(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    rh, cap = CFG["rounds_of_64"]
    count = rn.score_pnpl_scenes(st.sc, st.res.R, st.res.t, THRESH, status=st.res.status, usable=())   # the status mask excludes all
    assert not count.any()
    a = torch.arange(F, dtype=torch.int32, device=st.dev)
    R, t, s = (_rows(v, F, range(F), 64, 64) for v in (st.res.R, st.res.t, st.res.status))
    assert not rn.score_pnpl_active(st.sc, a, F, R, t, THRESH, status=s, usable=()).any()
    state, sim = _drive(st, count, rh, cap)
    assert (state.hyp_used == cap).all() and (state.head[:, 2] == 0).all() and (state.best == 0).all()
    _equals_the_fixed_selection(st, state, count, sim)   # head[f, 0], the pose and the masks of the fixed selection


def _snapshot(state, *more):
    return [v.clone() for v in (state.active, state.active_next, state.n_active, state.done, state.R, state.t, state.head, state.best, state.hyp_used,
                                state.mask, state.mask_lines) + more]


def _same(a, b):
    import torch

    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))   # bytes: a NaN equals itself


def test_nothing_active_and_entries_out_of_range_write_nothing(st):
    import torch

    from cvxpnpl_amd import _lib, ransac as rn
    from cvxpnpl_amd.api import _ptr

    rh, cap = CFG["rounds_of_64"]
    state, _ = _drive(st, st.count, rh, cap)
    state.done.fill_(7)
    before = _snapshot(state)
    # n_active = 0: nothing is launched
    R, t, s, c = (_rows(v, F, range(F), 0, 64) for v in (st.res.R, st.res.t, st.res.status, st.count))
    rn.update_pnpl_active(st.sc, state, 0, 0, cap, CONF, c[:0], R[:0], t[:0], s[:0], THRESH)
    rn.compact_active(st.sc, state, 0)
    Q, B = rn.sample_assemble_active(st.sc, state.active, 0, 0, 64, cap, st.order, POOL_FULL)
    assert Q.shape[0] == 0 and B.shape[0] == 0 and rn.score_pnpl_active(st.sc, state.active, 0, R[:0], t[:0], THRESH, status=s[:0]).shape[0] == 0
    torch.cuda.synchronize()
    assert _same(before, _snapshot(state))
    # entries outside [0, F): skipped, not clamped.  Three bad entries around one good one (scene 8).
    g8 = 8
    bad = torch.tensor([-1, F, g8, 2**31 - 1], dtype=torch.int32, device=st.dev)
    A, Hr = 4, 64
    state.active[:A] = bad
    R, t, s, c = (_rows(v, F, [0, 1, g8, 2], 128, Hr) for v in (st.res.R, st.res.t, st.res.status, st.count))
    L = _lib.ransac_pnpl_adaptive_lib()
    stream = C.c_void_p(torch.cuda.current_stream(st.dev).cuda_stream)
    sc = st.sc
    Q = torch.full((A * Hr, 45), -7.0, dtype=torch.float64, device=st.dev)
    B = torch.full((A * Hr, 27), -7.0, dtype=torch.float64, device=st.dev)
    idx = torch.full((A * Hr, 4), -7, dtype=torch.int32, device=st.dev)
    cnt = torch.full((A * Hr,), -7, dtype=torch.int32, device=st.dev)
    scene, data = (_ptr(sc.offsets), sc.total, _ptr(sc.line_offsets), sc.line_total), (_ptr(sc.x), _ptr(sc.X), _ptr(sc.l2), _ptr(sc.l3))
    assert L.cvxpnpl_ransac_pnpl_adaptive_sample_assemble(F, A, _ptr(bad), 128, Hr, cap, 0, *scene, _ptr(sc.seeds), None, *data, _ptr(sc.K), sc.per_scene_K,
                                                          _ptr(idx), _ptr(Q), _ptr(B), stream) == 0
    assert L.cvxpnpl_ransac_pnpl_adaptive_score(F, A, _ptr(bad), Hr, *scene, _ptr(R), _ptr(t), _ptr(s), 5, _ptr(sc.K), sc.per_scene_K, *data, THRESH,
                                                _ptr(cnt), stream) == 0
    torch.cuda.synchronize()
    good = slice(2 * Hr, 3 * Hr)
    for buf, ref in ((Q, st.Q), (B, st.B), (idx, st.idx), (cnt, st.count)):
        assert _bits(buf[good], _rows(ref, F, [g8], 128, Hr))
        rest = torch.cat([buf[:2 * Hr], buf[3 * Hr:]])
        assert (rest == -7).all()
    # the update: only scene 8 may change (its best can only grow), nothing of any other scene
    snap = _snapshot(state)
    rn.update_pnpl_active(st.sc, state, A, 128, cap, CONF, c, R, t, s, THRESH)
    torch.cuda.synchronize()
    now = _snapshot(state)
    rows = torch.as_tensor([f for f in range(F) if f != g8], device=st.dev)
    for x, y in zip(snap[4:9], now[4:9]):    # R, t, head, best, hyp_used
        assert torch.equal(x[rows].view(torch.uint8), y[rows].view(torch.uint8))
    for k, off in ((9, st.offp), (10, st.offl)):
        m0, m1 = snap[k].clone(), now[k].clone()
        m0[off[g8]:off[g8 + 1]] = 0; m1[off[g8]:off[g8 + 1]] = 0
        assert torch.equal(m0, m1)
    assert state.done[[0, 1, 3]].tolist() == [7, 7, 7] and int(state.done[2]) in (0, 1) and int(state.hyp_used[g8]) == 192
    # the compaction drops them whatever their (unwritten) done flags say
    state.done[:A] = 0
    rn.compact_active(st.sc, state, A)
    assert int(state.n_active.cpu()) == 1 and int(state.active_next[0]) == g8


def test_more_active_scenes_than_one_grid_dimension_holds():
    """66 000 scenes of 2 points and 2 lines, packed with sizes; rounds of 4 under a cap of 8: two slabs of the (hypotheses, entries) grids."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    dev = torch.device("cuda:0")
    nF, base, Hr, cap = 66000, 100, 4, 8
    K = np.array(synth.K_KINECT)
    ds = [synth.make_ransac_pnpl(2, 2, outlier_frac=0.5 * (j % 2), sigma=0.5, seed=700 + j, K=K) for j in range(base)]   # half of them clean
    tile = lambda key: np.tile(np.concatenate([d[key] for d in ds]), (nF // base,) + (1,) * (ds[0][key].ndim - 1))
    sc = rn.pack_pnpl_scenes(tile("pts_2d"), tile("line_2d"), tile("pts_3d"), tile("line_3d"), K, sizes=[2] * nF, line_sizes=[2] * nF, device=dev,
                             seeds=list(range(nF)))
    Qa, Ba, idx = rn.sample_assemble_scenes(sc, cap, want_idx=True)
    res = rn.solve_minimal_costs(Qa, Ba, eps=1e-6, max_iters=100)
    count = rn.score_pnpl_scenes(sc, res.R, res.t, THRESH, status=res.status, usable=(0, 2))
    sim = replay(count.cpu().numpy().reshape(nF, cap), res.status.cpu().numpy().reshape(nF, cap), [(2, 2)] * nF, CONF, Hr, cap)
    assert (sim["hyp_used"] == Hr).any() and (sim["hyp_used"] == cap).any() and len(sim["active"][1]) > 0
    state = rn.adaptive_pnpl_init(sc)
    A = nF
    for r, act in enumerate(sim["active"]):
        assert A == len(act) and np.array_equal(state.active[:A].cpu().numpy(), act)
        h0 = r * Hr
        Q, B, qi = rn.sample_assemble_active(sc, state.active, A, h0, Hr, cap, want_idx=True)
        assert torch.equal(qi, _rows(idx, nF, act, h0, Hr)) and _bits(Q, _rows(Qa, nF, act, h0, Hr)) and _bits(B, _rows(Ba, nF, act, h0, Hr))
        R, t, s = (_rows(v, nF, act, h0, Hr) for v in (res.R, res.t, res.status))
        c = rn.score_pnpl_active(sc, state.active, A, R, t, THRESH, status=s, usable=(0, 2))
        assert torch.equal(c, _rows(count, nF, act, h0, Hr))
        rn.update_pnpl_active(sc, state, A, h0, cap, CONF, c, R, t, s, THRESH)
        rn.compact_active(sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
    assert A == 0
    used = state.hyp_used.cpu().numpy()
    assert np.array_equal(used, sim["hyp_used"])
    for u in (Hr, cap):
        R1, t1, h1, mp1, ml1 = rn.select_pnpl_scenes(sc, *(_rows(v, nF, range(nF), 0, u) for v in (count, res.R, res.t, res.status)), THRESH)
        sel = torch.as_tensor(np.nonzero(used == u)[0], device=dev)
        assert torch.equal(state.head[sel], h1[sel]) and _bits(state.R[sel], R1[sel]) and _bits(state.t[sel], t1[sel])
        assert torch.equal(state.mask.reshape(nF, 2)[sel], mp1.reshape(nF, 2)[sel]) and torch.equal(state.mask_lines.reshape(nF, 2)[sel], ml1.reshape(nF, 2)[sel])


# ---- 4. the whole call ----------------------------------------------------------------------------------------------------------------------
def _project(R, t, K, X):
    Xc = X @ R.T + t
    uvw = Xc @ K.T
    with np.errstate(all="ignore"):
        return uvw[:, :2] / uvw[:, 2:3], Xc[:, 2]


def _borders(R, t, K, d, tol=1e-6):
    """(points, lines) within tol px of the threshold (or of depth 0) under the pose: where two poses 1e-8 rad apart may disagree"""
    bp, bl = np.zeros(len(d["pts_3d"]), bool), np.zeros(len(d["line_3d"]), bool)
    with np.errstate(all="ignore"):
        if len(bp):
            uv, depth = _project(R, t, K, d["pts_3d"])
            bp = (np.abs(np.linalg.norm(uv - d["pts_2d"], axis=-1) - THRESH) < tol) | (np.abs(depth) < 1e-9)
        if len(bl):
            L = len(bl)
            a, b = d["line_2d"][:, 0], d["line_2d"][:, 1]
            l = np.cross(np.concatenate([a, np.ones((L, 1))], 1), np.concatenate([b, np.ones((L, 1))], 1))
            uv, depth = _project(R, t, K, d["line_3d"].reshape(-1, 3))
            uv, depth = uv.reshape(L, 2, 2), depth.reshape(L, 2)
            dist = np.abs(uv[..., 0] * l[:, None, 0] + uv[..., 1] * l[:, None, 1] + l[:, None, 2]) / np.hypot(l[:, 0], l[:, 1])[:, None]
            bl = ((np.abs(dist - THRESH) < tol) | (np.abs(depth) < 1e-9)).any(-1)
    return bp, bl


def test_whole_call_equals_fixed_calls_at_the_budgets_used(st):
    """Per distinct hyp_used u, the scenes that stopped at u against ransac_pnpl_batch(n_hyp=u): the rules of the fixed-budget whole-call
    test of section 13 (masks equal apart from correspondences within 1e-6 px of the threshold, then poses to 1e-8, status and best_index
    equal; at most one scene set aside in all -- the solves run at another batch size and layout)."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    out = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=200, confidence=CONF, round_hyp=64, refit=False, **kw)
    used = out["hyp_used"].numpy()
    assert out["hyp_used"].dtype == torch.int32 and not out["hyp_used"].is_cuda and used.shape == (F,)
    assert out["rounds"] == 4 and out["confidence"] == CONF and out["n_hyp"] == 200 and "pool_full" not in out
    assert set(used.tolist()) <= {64, 128, 192, 200} and used.max() == 200
    print("whole call: hyp_used", used.tolist())
    mpa, mla = out["inliers_pts"].cpu().numpy(), out["inliers_lines"].cpu().numpy()
    Rb, tb = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    aside = []
    for u in sorted(set(used.tolist())):
        one = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=int(u), refit=False, **kw)
        R1, t1, mp1, ml1 = one["R"].cpu().numpy(), one["t"].cpu().numpy(), one["inliers_pts"].cpu().numpy(), one["inliers_lines"].cpu().numpy()
        for f in np.nonzero(used == u)[0]:
            sp, sl = slice(st.offp[f], st.offp[f + 1]), slice(st.offl[f], st.offl[f + 1])
            bp, bl = _borders(R1[f], t1[f], st.Kf[f], st.scenes[f])
            if ((mpa[sp] != mp1[sp]) & ~bp).any() or ((mla[sl] != ml1[sl]) & ~bl).any():
                aside.append(int(f))
                continue
            assert abs(int(out["n_inliers"][f]) - int(one["n_inliers"][f])) <= int(bp.sum() + bl.sum()), f
            assert int(out["n_inliers"][f]) == int(mpa[sp].sum() + mla[sl].sum()), f
            if np.array_equal(mpa[sp], mp1[sp]) and np.array_equal(mla[sl], ml1[sl]):
                if not (np.isfinite(R1[f]).all() and np.isfinite(t1[f]).all()):
                    assert np.array_equal(np.isfinite(Rb[f]), np.isfinite(R1[f])) and np.array_equal(np.isfinite(tb[f]), np.isfinite(t1[f])), f
                    continue
                geo = float(synth.geodesic(Rb[f], R1[f]))
                rel = float(np.abs(tb[f] - t1[f]).max() / max(np.abs(t1[f]).max(), 1e-300))
                assert geo <= 1e-8 and rel <= 1e-8, (f, geo, rel)
                assert int(out["status"][f]) == int(one["status"][f]) and int(out["best_index"][f]) == int(one["best_index"][f]), f
    print("whole call: set aside", aside)
    assert len(aside) <= 1, aside


KEYS = ("R", "t", "inliers_pts", "inliers_lines", "offsets", "line_offsets", "head")


def _same_out(a, b, more=()):
    return all(_bits(a[k], b[k]) for k in KEYS + tuple(more))


def test_whole_call_keys_determinism_streams_and_the_default(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    fixed_keys = {"R", "t", "inliers_pts", "offsets", "inliers_lines", "line_offsets", "n_inliers", "status", "n_certified", "best_index", "head",
                  "sizes", "line_sizes", "n_hyp"}
    # without the keywords: today's call, key for key and bit for bit
    d0 = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=128, **kw)
    d1 = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=128, confidence=None, round_hyp=7, quality=None, line_quality=None, pool_full=None, **kw)
    assert set(d0) == set(d1) == fixed_keys and _same_out(d0, d1)
    # pool_full = 0: the uniform sampler bit for bit, through the round sampler
    d2 = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=128, quality=st.qp, line_quality=st.ql, pool_full=0, **kw)
    assert set(d2) == fixed_keys | {"pool_full"} and d2["pool_full"] == 0 and _same_out(d0, d2)
    g = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=128, quality=st.qp, line_quality=st.ql, **kw)
    assert g["pool_full"] == 128

    def call(n, **more):
        a = [x[:n] for x in st.args]
        return rn.ransac_pnpl_batch(*a, st.K[:n] if st.per else st.K, n_hyp=200, confidence=CONF, round_hyp=64, quality=st.qp[:n], line_quality=st.ql[:n],
                                    pool_full=POOL_FULL, **more, **kw)

    full = call(F, refit=True, polish=True)
    assert set(full) == fixed_keys | {"refine", "hyp_used", "rounds", "confidence", "pool_full"}
    assert full["R"].shape == (F, 3, 3) and full["inliers_pts"].shape == (st.offp[-1],) and full["inliers_lines"].shape == (st.offl[-1],)
    assert full["hyp_used"].shape == (F,) and full["pool_full"] == POOL_FULL
    big = [f for f in range(F) if MS[f] >= 60]
    assert all(int(full["n_inliers"][f]) >= 0.3 * MS[f] for f in big)   # at most 0.6 of a scene is clutter: a consensus was found

    def same(a, b):
        return _same_out(a, b, ("hyp_used",)) and a["rounds"] == b["rounds"]

    a, b = call(F), call(F)
    assert same(a, b)   # two identical calls are bit-identical
    c = call(5)
    side = torch.cuda.Stream(device=st.dev)
    side.wait_stream(torch.cuda.current_stream(st.dev))
    with torch.cuda.stream(side):   # a call on a side stream directly followed by one of another F
        a2 = call(F)
        c2 = call(5)
    side.synchronize()
    assert same(a, a2) and same(c, c2)
    # the packed form, with the qualities packed as a host tensor and as a list of numbers, gives the same call
    packed = rn.ransac_pnpl_batch(*(np.concatenate(x) for x in st.args), st.K, n_hyp=200, confidence=CONF, round_hyp=64, sizes=[p for p, _ in SHAPES],
                                  line_sizes=[l for _, l in SHAPES], quality=torch.as_tensor(np.concatenate(st.qp)),
                                  line_quality=np.concatenate(st.ql).tolist(), pool_full=POOL_FULL, thresh=THRESH, seed=st.seeds, device=st.dev)
    assert same(a, packed)


def test_wrappers_return_scene_0_of_the_batch_call(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    kw = dict(n_hyp=200, confidence=CONF, round_hyp=64, pool_full=POOL_FULL, thresh=THRESH, device=st.dev)
    for f in (2, 8, 13):   # a mixed minimal scene, two mixed scenes
        p2, l2, p3, l3 = (a[f] for a in st.args)
        out = rn.ransac_pnpl_batch([p2], [l2], [p3], [l3], st.Kf[f], quality=[st.qp[f]], line_quality=[st.ql[f]], seed=st.seeds[f], **kw)
        one = rn.ransac_pnpl(p2, l2, p3, l3, st.Kf[f], quality=st.qp[f], line_quality=st.ql[f], seed=st.seeds[f], **kw)
        assert _bits(one["R"], out["R"][0]) and _bits(one["t"], out["t"][0]), f
        assert torch.equal(one["inliers_pts"], out["inliers_pts"]) and torch.equal(one["inliers_lines"], out["inliers_lines"]), f
        assert [one["status"], one["n_inliers"], one["best_index"], one["n_certified"]] == out["head"][0].tolist(), f
        assert isinstance(one["hyp_used"], int) and one["hyp_used"] == int(out["hyp_used"][0]) and one["rounds"] == out["rounds"], f
        assert one["confidence"] == CONF and one["pool_full"] == POOL_FULL and one["n_hyp"] == 200
    lines_only = [f for f, (p, l) in enumerate(SHAPES) if p == 0]
    assert len(lines_only) >= 3
    l2, l3, ql = ([x[f] for f in lines_only] for x in (st.args[1], st.args[3], st.ql))
    Kl = st.K[lines_only] if st.per else st.K
    a = rn.ransac_pnl_batch(l2, l3, Kl, line_quality=ql, seed=7, **kw)
    b = rn.ransac_pnpl_batch(None, l2, None, l3, Kl, line_quality=ql, seed=7, **kw)
    assert _same_out(a, b, ("hyp_used",)) and a["inliers_pts"].numel() == 0 and a["sizes"] == (0,) * len(lines_only)
    one = rn.ransac_pnl(l2[2], l3[2], Kl[2] if st.per else Kl, line_quality=ql[2], seed=9, **kw)
    lo = a["line_offsets"].cpu().numpy()
    assert torch.equal(one["inliers_lines"], a["inliers_lines"][lo[2]:lo[3]]) and one["n_inliers"] == int(a["n_inliers"][2])
    assert one["hyp_used"] == int(a["hyp_used"][2])


# ---- 5. points only -------------------------------------------------------------------------------------------------------------------------
def test_point_only_scenes_agree_with_ransac_pnp_batch(st):
    """ransac_pnpl_batch(confidence=, quality=) on scenes without lines against ransac_pnp_batch(confidence=, quality=): hyp_used, winners
    and counts equal, poses within the 1e-8 rad of the fixed-budget point-only comparison (tests/test_ransac_pnpl_gpu.py)."""
    from cvxpnpl_amd import ransac as rn, synth
    from ransac_guided_reference import planted_quality

    sizes = [4, 7, 47, 70, 129, 250, 600, 33]
    xs, Xs, qs = [], [], []
    rs = np.random.RandomState(23)
    for i, m in enumerate(sizes):
        d = synth.make_ransac(1, n_corr=m, outlier_frac=0.6 * i / len(sizes) if m > 8 else 0.0, sigma=0.5, seed=900 + i)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); qs.append(planted_quality(d["inlier"], rs))
    K = np.stack([st.Kf[f] for f in range(len(sizes))]) if st.per else st.K
    kw = dict(n_hyp=200, thresh=THRESH, seed=SEED, device=st.dev, confidence=CONF, round_hyp=64, quality=qs, pool_full=POOL_FULL)
    ref = rn.ransac_pnp_batch(xs, Xs, K, **kw)
    out = rn.ransac_pnpl_batch(xs, None, Xs, None, K, **kw)
    assert out["inliers_lines"].numel() == 0 and out["rounds"] == ref["rounds"] and out["pool_full"] == ref["pool_full"] == POOL_FULL
    print("points only: hyp_used", out["hyp_used"].tolist())
    assert np.array_equal(out["hyp_used"].numpy(), ref["hyp_used"].numpy()), (out["hyp_used"], ref["hyp_used"])
    assert np.array_equal(out["best_index"].numpy(), ref["best_index"].numpy()), (out["best_index"], ref["best_index"])
    assert np.array_equal(out["n_inliers"].numpy(), ref["n_inliers"].numpy()), (out["n_inliers"], ref["n_inliers"])
    off = np.concatenate([[0], np.cumsum(sizes)])
    Ra, Rb = out["R"].cpu().numpy(), ref["R"].cpu().numpy()
    tb = ref["t"].cpu().numpy()
    ma, mb = out["inliers_pts"].cpu().numpy(), ref["inliers"].cpu().numpy()
    worst = 0.0
    for f, m in enumerate(sizes):
        Kf = K[f] if st.per else K
        uv, depth = _project(Rb[f], tb[f], Kf, Xs[f])
        err = np.linalg.norm(uv - xs[f], axis=-1)
        border = (np.abs(err - THRESH) < 1e-6) | (np.abs(depth) < 1e-9)   # (the two poses differ by up to 1e-8 rad: ~1e-6 px)
        assert not ((ma[off[f]:off[f + 1]] != mb[off[f]:off[f + 1]]) & ~border).any(), f
        if np.isfinite(Rb[f]).all():
            worst = max(worst, float(synth.geodesic(Ra[f], Rb[f])))
    print(f"points only, adaptive and guided: max geodesic between ransac_pnpl_batch and ransac_pnp_batch {worst:.3e} rad")
    assert worst <= 1e-8, worst


# ---- 6. guided, deterministic ---------------------------------------------------------------------------------------------------------------
def test_a_quality_that_knows_four_inliers_finds_the_pose_at_hypothesis_0():
    """50 points and 50 lines, noise-free inliers, 70 % clutter; the quality ranks two inlier points and two inlier lines first.  Hypothesis
    0 draws exactly those four, no later hypothesis counts more, and with confidence = 0.99 the scene stops after its first round:
    30 inliers of 100 need N = log(0.01) / log1p(-q) = 657 hypotheses, q = 30 29 28 27 / (100 99 98 97), under a round of 700."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth
    from ransac_adaptive_reference import needed

    dev = torch.device("cuda:0")
    P = L = 50
    d = synth.make_ransac_pnpl(P, L, outlier_frac=0.7, sigma=0.0, seed=4242)
    ip, il = np.nonzero(d["inlier_pts"])[0], np.nonzero(d["inlier_lines"])[0]
    assert len(ip) == 15 and len(il) == 15 and 600 < needed(30, 100, CONF) < 700
    rs = np.random.RandomState(3)
    qp, ql = rs.uniform(0.0, 0.9, P), rs.uniform(0.0, 0.9, L)     # nothing else is told apart
    qp[ip[[3, 11]]] = 1.0
    ql[il[[0, 7]]] = 1.0
    four = sorted([int(ip[3]), int(ip[11]), P + int(il[0]), P + int(il[7])])
    sc = rn.pack_pnpl_scenes([d["pts_2d"]], [d["line_2d"]], [d["pts_3d"]], [d["line_3d"]], d["K"], device=dev, seeds=[5])
    order = rn.rank_pnpl_scenes(sc, torch.as_tensor(qp).to(dev), torch.as_tensor(ql).to(dev))
    assert sorted(order[:4].tolist()) == four
    _, _, idx = rn.sample_assemble_active(sc, torch.zeros(1, dtype=torch.int32, device=dev), 1, 0, 8, 8, order, 8, want_idx=True)
    assert sorted(idx[0].tolist()) == four                        # hypothesis 0 draws exactly those four
    args = (d["pts_2d"], d["line_2d"], d["pts_3d"], d["line_3d"], d["K"])
    kw = dict(quality=qp, line_quality=ql, thresh=THRESH, seed=5, device=dev, refit=False)
    fixed = rn.ransac_pnpl(*args, n_hyp=256, **kw)
    assert fixed["best_index"] == 0 and fixed["n_inliers"] >= 30 and fixed["status"] in (0, 2)
    assert float(synth.geodesic(fixed["R"].cpu().numpy(), d["R_gt"])) < 1e-3
    ada = rn.ransac_pnpl(*args, n_hyp=2100, confidence=CONF, round_hyp=700, **kw)
    assert ada["best_index"] == 0 and ada["rounds"] == 1 and ada["hyp_used"] == 700 and ada["n_inliers"] >= 30
    mp, ml = ada["inliers_pts"].cpu().numpy(), ada["inliers_lines"].cpu().numpy()
    assert (mp | ~d["inlier_pts"]).all() and (ml | ~d["inlier_lines"]).all()   # every planted inlier is in the masks
