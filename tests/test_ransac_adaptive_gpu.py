"""Adaptive RANSAC: a hypothesis budget per scene, solved in rounds (ransac_pnp_batch(confidence=...), libcvxpnpl_amd_ransac_adaptive.so;
DESIGN.md section 19).

Every stage is held against the third library's kernel on the same inputs (sample_scenes, score_scenes, select_scenes: the fixed-budget
path, which this feature does not touch) and the bookkeeping against the numpy replay of tests/ransac_adaptive_reference.py; then the
whole call against fixed-budget calls at the budgets it stopped at.  14 scenes of 4 .. 700 correspondences (exactly 4, around the wave
width 64 and around the scoring tile of 512), outlier shares 0 .. 0.6, sigma 0.5 px; once with a shared K and once with a K per scene."""
import ctypes as C

import numpy as np
import pytest

from ransac_adaptive_reference import simulate

pytestmark = pytest.mark.gpu

SIZES = [4, 4, 5, 63, 64, 65, 100, 100, 100, 511, 512, 513, 700, 700]
OUTLIERS = [0.0, 0.25, 0.2, 0.1, 0.3, 0.5, 0.3, 0.45, 0.6, 0.0, 0.2, 0.4, 0.55, 0.6]   # (0.25 of 4: one displaced point)
F, THRESH, SEED, CONF = len(SIZES), 2.0, 2000, 0.99
CFG = {"rounds_of_64": (64, 200), "two_workgroups": (300, 600)}   # (round_hyp, cap); 300 = one full workgroup in x and a partial one
H_ALL = 600   # hypotheses solved once per scene: both caps are prefixes of them


def _make_scenes(per_scene_K, sizes=SIZES, outliers=OUTLIERS, seed0=300):
    from cvxpnpl_amd import synth

    xs, Xs, Ks = [], [], []
    n = len(sizes)
    for f, m in enumerate(sizes):
        K = np.array(synth.K_KINECT)
        if per_scene_K:
            K[0, 0] *= 0.8 + 0.4 * f / max(n - 1, 1)
            K[1, 1] *= 0.8 + 0.4 * f / max(n - 1, 1)
        d = synth.make_ransac(1, n_corr=m, outlier_frac=outliers[f], sigma=0.5, seed=seed0 + f, K=K)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); Ks.append(K)
    return xs, Xs, (np.stack(Ks) if per_scene_K else Ks[0])


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One frame set per K mode, computed once: scenes, H_ALL minimal sets per scene by the third library's sampler, their solves and
    counts.  Nothing below changes it."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_lib(); _lib.ransac_adaptive_lib()
    s = _State()
    s.dev = torch.device("cuda:0")
    s.per = request.param == "per_scene_K"
    s.xs, s.Xs, s.K = _make_scenes(s.per)
    s.seeds = [SEED + f for f in range(F)]
    s.sc = rn.pack_scenes(s.xs, s.Xs, s.K, device=s.dev, seeds=s.seeds)
    s.off = np.concatenate([[0], np.cumsum(SIZES)])
    s.p2, s.p3, s.Kh, s.idx = rn.sample_scenes(s.sc, H_ALL, want_idx=True)
    s.res = ca.pnp_batch(s.p2, s.p3, s.Kh if s.per else s.sc.K, eps=1e-6, max_iters=100)
    s.count = rn.score_scenes(s.sc, s.res.R, s.res.t, THRESH, status=s.res.status, usable=(0, 2))
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


def _margins_hold(sim):
    """The condition under which a last-bit difference between the device's and numpy's log cannot flip a decision."""
    for f, r, drawn, N in sim["margins"]:
        if np.isfinite(N):
            assert abs(drawn - N) > 1e-6 * max(N, 1.0), f"scene {f} round {r}: drawn {drawn} against N {N}: change the seed"


def test_the_reference_sees_every_path(st):
    """From the reference alone, on the fixed counts: the configuration exercises a first-round stop, a middle-round stop, a run to the
    cap, and the short last round."""
    rh, cap = CFG["rounds_of_64"]
    sim = simulate(st.count_h, st.status_h, SIZES, CONF, rh, cap)
    _margins_hold(sim)
    used = sim["hyp_used"]
    print("hyp_used", list(used), "best", list(sim["best"]), "active per round", [len(a) for a in sim["active"]])
    assert (used == 64).any()                                   # a scene stopping in round 1
    assert ((used == 128) | (used == 192)).any()                # ... in a middle round
    assert (used == cap).any()                                  # ... running to the cap
    assert len(sim["active"]) == 4 and cap - 3 * rh == 8        # the last round is short: Hr = 8
    rh2, cap2 = CFG["two_workgroups"]
    sim2 = simulate(st.count_h, st.status_h, SIZES, CONF, rh2, cap2)
    _margins_hold(sim2)
    assert len(sim2["active"]) == 2 and (sim2["hyp_used"] == 300).any() and (sim2["hyp_used"] == 600).any()


@pytest.mark.parametrize("h0", [0, 64, 192])
def test_sampler_draws_the_rows_of_the_fixed_sampler(st, h0):
    import torch

    from cvxpnpl_amd import ransac as rn

    lists = {"identity": list(range(F)), "every_other": list(range(0, F, 2)), "one": [F - 3], "reversed": list(range(F - 1, -1, -1))}
    for rh, cap in CFG.values():
        if h0 >= cap:
            continue
        Hr = min(rh, cap - h0)
        for name, act in lists.items():
            a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
            p2, p3, Kh, idx = rn.sample_active(st.sc, a, len(act), h0, Hr, cap, want_idx=True)
            assert idx.shape == (len(act) * Hr, 4) and p2.shape == (len(act) * Hr, 4, 2) and p3.shape == (len(act) * Hr, 4, 3)
            assert torch.equal(idx, _rows(st.idx, F, act, h0, Hr)), (name, rh)
            assert torch.equal(p2, _rows(st.p2, F, act, h0, Hr)) and torch.equal(p3, _rows(st.p3, F, act, h0, Hr)), (name, rh)
            assert (Kh is None) == (not st.per)
            if st.per:
                assert torch.equal(Kh, _rows(st.Kh, F, act, h0, Hr)), (name, rh)
    # a longer tensor than n_active: only the first n_active entries count
    a = torch.as_tensor(list(range(F)), dtype=torch.int32, device=st.dev)
    p2, _, _ = rn.sample_active(st.sc, a, 3, h0, 8, 200)
    assert torch.equal(p2, _rows(st.p2, F, [0, 1, 2], h0, 8))


def test_scoring_equals_the_rows_of_the_fixed_scoring(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    differing = 0
    for act in (list(range(F)), list(range(1, F, 2)), [F - 1], list(range(F - 1, -1, -1))):
        a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
        for h0, Hr in ((0, 64), (192, 8), (0, 300), (300, 300)):
            R, t, s = (_rows(v, F, act, h0, Hr) for v in (st.res.R, st.res.t, st.res.status))
            mine = rn.score_active(st.sc, a, len(act), R, t, THRESH, status=s, usable=(0, 2))
            differing += int((mine != _rows(st.count, F, act, h0, Hr)).sum())
    assert differing == 0, differing   # the same predicate on the same poses


def _drive(st, count, rh, cap, sim=None, status=None):
    """The rounds on given counts [F * H_ALL] (device int32): update + compact per round, the active list held against the replay at every
    round.  Returns (state, replay)."""
    import torch

    from cvxpnpl_amd import ransac as rn

    status = st.res.status if status is None else status
    if sim is None:
        sim = simulate(count.cpu().numpy().reshape(F, H_ALL), status.cpu().numpy().reshape(F, H_ALL), SIZES, CONF, rh, cap)
    _margins_hold(sim)
    state = rn.adaptive_init(st.sc)
    assert torch.equal(state.head.cpu(), torch.tensor([[3, -1, 0, 0]] * F, dtype=torch.int32)) and int(state.n_active.cpu()) == F
    assert not state.hyp_used.any() and (state.best == -1).all()
    A, h0 = F, 0
    for r, act in enumerate(sim["active"]):
        assert A == len(act), (r, A, list(act))
        assert np.array_equal(state.active[:A].cpu().numpy(), act), (r, list(act))
        Hr = min(rh, cap - h0)
        R, t, s, c = (_rows(v, F, act, h0, Hr) for v in (st.res.R, st.res.t, status, count))
        rn.update_active(st.sc, state, A, h0, cap, CONF, c, R, t, s, THRESH)
        rn.compact_active(st.sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
        h0 += Hr
    assert A == 0, A
    return state, sim


def _equals_the_fixed_selection(st, state, count, sim, status=None):
    """hyp_used against the replay; pose, head and mask bit for bit against select_scenes over each scene's first hyp_used hypotheses."""
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
        R1, t1, h1, m1 = rn.select_scenes(st.sc, c, R, t, s, THRESH)
        for f in np.nonzero(used == u)[0]:
            assert torch.equal(state.head[f], h1[f]), (f, u, state.head[f].tolist(), h1[f].tolist())
            assert torch.equal(state.R[f].view(torch.int64), R1[f].view(torch.int64)), (f, u)   # bit for bit (as words: a NaN pose equals itself)
            assert torch.equal(state.t[f].view(torch.int64), t1[f].view(torch.int64)), (f, u)
            assert torch.equal(state.mask[st.off[f]:st.off[f + 1]], m1[st.off[f]:st.off[f + 1]]), (f, u)


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
    assert int(state.hyp_used.min()) == 64 and int(state.hyp_used.max()) == cap   # (4 of 4 stops at once, 4 of 700 never)
    _equals_the_fixed_selection(st, state, c, sim)


def test_a_scene_without_a_usable_hypothesis_runs_to_the_cap(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    rh, cap = CFG["rounds_of_64"]
    count = rn.score_scenes(st.sc, st.res.R, st.res.t, THRESH, status=st.res.status, usable=())   # the status mask excludes all
    assert not count.any()
    a = torch.arange(F, dtype=torch.int32, device=st.dev)
    R, t, s = (_rows(v, F, range(F), 64, 64) for v in (st.res.R, st.res.t, st.res.status))
    assert not rn.score_active(st.sc, a, F, R, t, THRESH, status=s, usable=()).any()
    state, sim = _drive(st, count, rh, cap)
    assert (state.hyp_used == cap).all() and (state.head[:, 2] == 0).all() and (state.best == 0).all()
    _equals_the_fixed_selection(st, state, count, sim)   # head[f, 0], the pose and the mask of the fixed selection


def _snapshot(state, *more):
    return [v.clone() for v in (state.active, state.active_next, state.n_active, state.done, state.R, state.t, state.head, state.best, state.mask,
                                state.hyp_used) + more]


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
    rn.update_active(st.sc, state, 0, 0, cap, CONF, c[:0], R[:0], t[:0], s[:0], THRESH)
    rn.compact_active(st.sc, state, 0)
    p2, p3, Kh = rn.sample_active(st.sc, state.active, 0, 0, 64, cap)
    assert p2.shape[0] == 0 and rn.score_active(st.sc, state.active, 0, R[:0], t[:0], THRESH, status=s[:0]).shape[0] == 0
    torch.cuda.synchronize()
    assert _same(before, _snapshot(state))
    # entries outside [0, F): skipped, not clamped.  Three bad entries around one good one (scene 6).
    bad = torch.tensor([-1, F, 6, 2**31 - 1], dtype=torch.int32, device=st.dev)
    A, Hr = 4, 64
    state.active[:A] = bad
    R, t, s, c = (_rows(v, F, [0, 1, 6, 2], 128, Hr) for v in (st.res.R, st.res.t, st.res.status, st.count))
    L = _lib.ransac_adaptive_lib()
    stream = C.c_void_p(torch.cuda.current_stream(st.dev).cuda_stream)
    sc = st.sc
    p2 = torch.full((A * Hr, 4, 2), -7.0, dtype=torch.float64, device=st.dev)
    p3 = torch.full((A * Hr, 4, 3), -7.0, dtype=torch.float64, device=st.dev)
    Kh = torch.full((A * Hr, 3, 3), -7.0, dtype=torch.float64, device=st.dev)
    idx = torch.full((A * Hr, 4), -7, dtype=torch.int32, device=st.dev)
    cnt = torch.full((A * Hr,), -7, dtype=torch.int32, device=st.dev)
    assert L.cvxpnpl_ransac_adaptive_sample(F, A, _ptr(bad), 128, Hr, cap, _ptr(sc.offsets), sc.total, _ptr(sc.seeds), _ptr(sc.x), _ptr(sc.X),
                                            _ptr(sc.K) if st.per else None, _ptr(idx), _ptr(p2), _ptr(p3), _ptr(Kh) if st.per else None, stream) == 0
    assert L.cvxpnpl_ransac_adaptive_score(F, A, _ptr(bad), Hr, _ptr(sc.offsets), sc.total, _ptr(R), _ptr(t), _ptr(s), 5, _ptr(sc.K), sc.per_scene_K,
                                           _ptr(sc.x), _ptr(sc.X), THRESH, _ptr(cnt), stream) == 0
    torch.cuda.synchronize()
    good = slice(2 * Hr, 3 * Hr)
    for buf, ref in ((p2, st.p2), (p3, st.p3), (idx, st.idx), (cnt, st.count)) + (((Kh, st.Kh),) if st.per else ()):
        assert torch.equal(buf[good], _rows(ref, F, [6], 128, Hr))
        rest = torch.cat([buf[:2 * Hr], buf[3 * Hr:]])
        assert (rest == -7).all()
    # the update: only scene 6 may change (it had stopped earlier or not: its best can only grow), nothing of any other scene
    snap = _snapshot(state)
    rn.update_active(st.sc, state, A, 128, cap, CONF, c, R, t, s, THRESH)
    torch.cuda.synchronize()
    now = _snapshot(state)
    keep = [f for f in range(F) if f != 6]
    rows = torch.as_tensor(keep, device=st.dev)
    for x, y in zip(snap[4:8] + snap[9:], now[4:8] + now[9:]):    # R, t, head, best, hyp_used
        assert torch.equal(x[rows].view(torch.uint8), y[rows].view(torch.uint8))
    m0, m1 = snap[8].clone(), now[8].clone()
    m0[st.off[6]:st.off[7]] = 0; m1[st.off[6]:st.off[7]] = 0
    assert torch.equal(m0, m1)
    assert state.done[[0, 1, 3]].tolist() == [7, 7, 7] and int(state.done[2]) in (0, 1) and int(state.hyp_used[6]) == 192
    # the compaction drops them whatever their (unwritten) done flags say
    state.done[:A] = 0
    rn.compact_active(st.sc, state, A)
    assert int(state.n_active.cpu()) == 1 and int(state.active_next[0]) == 6


def test_compaction_is_stable_and_repeatable(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    n = 1000   # four chunks of 256, the last partial
    sizes = [4] * n
    rs = np.random.RandomState(5)
    sc = rn.pack_scenes(rs.random_sample((4 * n, 2)), rs.random_sample((4 * n, 3)), np.eye(3), sizes=sizes, device=st.dev, seeds=list(range(n)))
    state = rn.adaptive_init(sc)
    perm = rs.permutation(n).astype(np.int32)
    done = (rs.rand(n) < 0.4).astype(np.int32)
    state.active.copy_(torch.as_tensor(perm))
    for A in (n, 999, 513, 512, 257, 256, 255, 65, 64, 1):
        state.done[:A] = torch.as_tensor(done[:A], device=st.dev)
        outs = []
        for _ in range(2):
            state.active_next.fill_(-5)
            rn.compact_active(sc, state, A)
            outs.append((state.active_next.cpu().numpy().copy(), int(state.n_active.cpu())))
        ref = perm[:A][done[:A] == 0]
        assert outs[0][1] == outs[1][1] == len(ref) and np.array_equal(outs[0][0], outs[1][0]), A
        assert np.array_equal(outs[0][0][:len(ref)], ref) and (outs[0][0][len(ref):] == -5).all(), A


def test_more_active_scenes_than_one_grid_dimension_holds():
    """66 000 scenes of 4 points, rounds of one hypothesis, cap 2: two slabs of the (hypotheses, scenes) grids."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn, synth

    dev = torch.device("cuda:0")
    nF, base = 66000, 100
    K = np.array(synth.K_KINECT)
    b2, b3 = [], []
    for j in range(base):   # half of the scenes clean, half with a displaced point
        d = synth.make_ransac(1, n_corr=4, outlier_frac=0.25 * (j % 2), sigma=0.5, seed=700 + j, K=K)
        b2.append(d["scene_2d"]); b3.append(d["scene_3d"])
    x = np.tile(np.concatenate(b2), (nF // base, 1))
    X = np.tile(np.concatenate(b3), (nF // base, 1))
    sc = rn.pack_scenes(x, X, K, sizes=[4] * nF, device=dev, seeds=list(range(nF)))
    p2, p3, _, idx = rn.sample_scenes(sc, 2, want_idx=True)
    res = ca.pnp_batch(p2, p3, sc.K, eps=1e-6, max_iters=100)
    count = rn.score_scenes(sc, res.R, res.t, THRESH, status=res.status, usable=(0, 2))
    sim = simulate(count.cpu().numpy().reshape(nF, 2), res.status.cpu().numpy().reshape(nF, 2), [4] * nF, CONF, 1, 2)
    assert (sim["hyp_used"] == 1).any() and (sim["hyp_used"] == 2).any()
    state = rn.adaptive_init(sc)
    A = nF
    for r, act in enumerate(sim["active"]):
        assert A == len(act) and np.array_equal(state.active[:A].cpu().numpy(), act)
        a = torch.as_tensor(act, device=dev)
        rows = a * 2 + r
        q2, q3, _, qi = rn.sample_active(sc, state.active, A, r, 1, 2, want_idx=True)
        assert torch.equal(qi, idx[rows]) and torch.equal(q2, p2[rows]) and torch.equal(q3, p3[rows])
        R, t, s = res.R[rows].contiguous(), res.t[rows].contiguous(), res.status[rows].contiguous()
        c = rn.score_active(sc, state.active, A, R, t, THRESH, status=s, usable=(0, 2))
        assert torch.equal(c, count[rows])
        rn.update_active(sc, state, A, r, 2, CONF, c, R, t, s, THRESH)
        rn.compact_active(sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
    assert A == 0
    used = state.hyp_used.cpu().numpy()
    assert np.array_equal(used, sim["hyp_used"])
    v = lambda full, u: full.reshape((nF, 2) + tuple(full.shape[1:]))[:, :u].reshape((nF * u,) + tuple(full.shape[1:])).contiguous()
    for u in (1, 2):
        R1, t1, h1, m1 = rn.select_scenes(sc, v(count, u), v(res.R, u), v(res.t, u), v(res.status, u), THRESH)
        sel = torch.as_tensor(np.nonzero(used == u)[0], device=dev)
        assert torch.equal(state.head[sel], h1[sel])
        assert torch.equal(state.R[sel].view(torch.int64), R1[sel].view(torch.int64)) and torch.equal(state.t[sel].view(torch.int64), t1[sel].view(torch.int64))
        assert torch.equal(state.mask.reshape(nF, 4)[sel], m1.reshape(nF, 4)[sel])


def _reproj(R, t, K, x, X):
    Xc = X @ R.T + t
    uvw = Xc @ K.T
    with np.errstate(all="ignore"):
        return np.linalg.norm(uvw[:, :2] / uvw[:, 2:3] - x, axis=-1)


def test_whole_call_equals_fixed_calls_at_the_budgets_used(st):
    """Per distinct hyp_used u, the scenes that stopped at u against ransac_pnp_batch(n_hyp=u): the rules of the fixed-budget whole-call
    test (masks equal apart from correspondences within 1e-6 px of the threshold, then poses to 1e-8, status and best_index equal; at most
    one scene set aside in all -- the solves run at another batch size and layout)."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    out = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, refit=False, **kw)
    used = out["hyp_used"].numpy()
    assert out["hyp_used"].dtype == torch.int32 and not out["hyp_used"].is_cuda and used.shape == (F,)
    assert out["rounds"] == 4 and out["confidence"] == CONF and out["n_hyp"] == 200
    assert set(used.tolist()) <= {64, 128, 192, 200} and used.max() == 200
    print("whole call: hyp_used", used.tolist())
    off, inl = st.off, out["inliers"].cpu().numpy()
    Rb, tb = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    aside = []
    for u in sorted(set(used.tolist())):
        one = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=int(u), refit=False, **kw)
        R1, t1, m1 = one["R"].cpu().numpy(), one["t"].cpu().numpy(), one["inliers"].cpu().numpy()
        for f in np.nonzero(used == u)[0]:
            Kf = st.K[f] if st.per else st.K
            mb, mf = inl[off[f]:off[f + 1]], m1[off[f]:off[f + 1]]
            border = np.abs(_reproj(R1[f], t1[f], Kf, st.xs[f], st.Xs[f]) - THRESH) < 1e-6
            if ((mb != mf) & ~border).any():
                aside.append(int(f))
                continue
            assert abs(int(out["n_inliers"][f]) - int(one["n_inliers"][f])) <= int(border.sum()), f
            assert int(out["n_inliers"][f]) == int(mb.sum()), f
            if np.array_equal(mb, mf):
                if not (np.isfinite(R1[f]).all() and np.isfinite(t1[f]).all()):
                    assert np.array_equal(np.isfinite(Rb[f]), np.isfinite(R1[f])) and np.array_equal(np.isfinite(tb[f]), np.isfinite(t1[f])), f
                    continue
                geo = float(synth.geodesic(Rb[f], R1[f]))
                rel = float(np.abs(tb[f] - t1[f]).max() / max(np.abs(t1[f]).max(), 1e-300))
                assert geo <= 1e-8 and rel <= 1e-8, (f, geo, rel)
                assert int(out["status"][f]) == int(one["status"][f]) and int(out["best_index"][f]) == int(one["best_index"][f]), f
    print("whole call: set aside", aside)
    assert len(aside) <= 1, aside


def test_whole_call_keys_determinism_streams_and_the_default(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    full = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, refit=True, polish=True, **kw)
    fixed_keys = {"R", "t", "inliers", "offsets", "n_inliers", "status", "n_certified", "best_index", "head", "sizes", "n_hyp", "refine"}
    assert set(full) == fixed_keys | {"hyp_used", "rounds", "confidence"}
    assert full["R"].shape == (F, 3, 3) and full["inliers"].shape == (sum(SIZES),) and full["hyp_used"].shape == (F,)
    big = [f for f in range(F) if SIZES[f] >= 63]
    assert all(int(full["n_inliers"][f]) >= 0.3 * SIZES[f] for f in big)   # at most 0.6 of a scene is clutter: a consensus was found

    def call(n):
        return rn.ransac_pnp_batch(st.xs[:n], st.Xs[:n], st.K[:n] if st.per else st.K, n_hyp=200, confidence=CONF, round_hyp=64, **kw)

    def same(a, b):
        return all(torch.equal(a[k], b[k]) for k in ("R", "t", "inliers", "offsets", "head", "hyp_used")) and a["rounds"] == b["rounds"]

    a, b = call(F), call(F)
    assert same(a, b)   # two identical adaptive calls are bit-identical
    c = call(5)
    side = torch.cuda.Stream(device=st.dev)
    side.wait_stream(torch.cuda.current_stream(st.dev))
    with torch.cuda.stream(side):   # an adaptive call on a side stream directly followed by one of another F
        a2 = call(F)
        c2 = call(5)
    side.synchronize()
    assert same(a, a2) and same(c, c2)
    # confidence=None is the call without the keyword
    d0 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, **kw)
    d1 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, confidence=None, round_hyp=7, **kw)
    assert set(d0) == set(d1) and all(torch.equal(d0[k], d1[k]) for k in ("R", "t", "inliers", "offsets", "head"))
