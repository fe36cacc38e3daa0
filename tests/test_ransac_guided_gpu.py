"""Guided RANSAC: minimal sets drawn from the best-ranked correspondences first (ransac_pnp_batch(quality=...),
libcvxpnpl_amd_ransac_guided.so).

The ranking and both samplers are held against the numpy reference of tests/ransac_guided_reference.py exactly, the round sampler against
the rows of the fixed one bit for bit, and the whole call against the calls it must equal.  14 scenes of 4 .. 700 correspondences
(4 and 5, where the pool is pinned, and the edges of the ranking's 256-lane tile), clutter 0 .. 0.6, sigma 0.5 px; once with a shared K
and once with a K per scene."""
import ctypes as C

import numpy as np
import pytest

from ransac_guided_reference import first_all_inlier, guided_sets, planted_quality, quality_patterns, rank

pytestmark = pytest.mark.gpu

SIZES = [4, 4, 5, 63, 64, 65, 100, 255, 256, 257, 511, 512, 513, 700]
OUTLIERS = [0.0, 0.25, 0.2, 0.1, 0.3, 0.5, 0.3, 0.45, 0.6, 0.0, 0.2, 0.4, 0.55, 0.6]   # (0.25 of 4: one displaced point)
F, THRESH, SEED, CONF = len(SIZES), 2.0, 2000, 0.99
POOLS = (0, 1, 7, 200, 10**6)
H_FIX = 200
CFG = {"rounds_of_64": (64, 200), "two_workgroups": (300, 600)}   # (round_hyp, cap); 300 = one full workgroup in x and a partial one
H_ALL = 600   # both caps are prefixes of it
GUARD = 64


def _make_scenes(per_scene_K):
    from cvxpnpl_amd import synth

    xs, Xs, Ks, inl = [], [], [], []
    for f, m in enumerate(SIZES):
        K = np.array(synth.K_KINECT)
        if per_scene_K:
            K[0, 0] *= 0.8 + 0.4 * f / (F - 1)
            K[1, 1] *= 0.8 + 0.4 * f / (F - 1)
        d = synth.make_ransac(1, n_corr=m, outlier_frac=OUTLIERS[f], sigma=0.5, seed=300 + f, K=K)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); Ks.append(K); inl.append(d["inlier"])
    return xs, Xs, (np.stack(Ks) if per_scene_K else Ks[0]), inl


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One frame set per K mode, computed once: scenes, their qualities and ranking, and H_ALL guided minimal sets per scene for every
    pool_full.  Nothing below changes it."""
    import torch

    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_lib(); _lib.ransac_adaptive_lib(); _lib.ransac_guided_lib()
    s = _State()
    s.dev = torch.device("cuda:0")
    s.per = request.param == "per_scene_K"
    s.xs, s.Xs, s.K, s.inl = _make_scenes(s.per)
    s.seeds = [SEED + f for f in range(F)]
    s.sc = rn.pack_scenes(s.xs, s.Xs, s.K, device=s.dev, seeds=s.seeds)
    s.off = np.concatenate([[0], np.cumsum(SIZES)])
    rs = np.random.RandomState(17)
    s.q = [planted_quality(a, rs) for a in s.inl]
    s.order_ref = [rank(q) for q in s.q]
    s.order = rn.rank_scenes(s.sc, torch.as_tensor(np.concatenate(s.q), device=s.dev))
    s.fix = {pf: rn.sample_scenes_guided(s.sc, H_ALL, s.order, pf, want_idx=True) for pf in POOLS}
    torch.cuda.synchronize()
    return s


def _rows(full, n_scenes, act, h0, Hr):
    """rows [f, h0 : h0 + Hr] for f in act of a tensor laid out [n_scenes * H, ...], as one contiguous [len(act) * Hr, ...] tensor"""
    import torch

    H = full.shape[0] // n_scenes
    v = full.reshape((n_scenes, H) + tuple(full.shape[1:]))
    a = torch.as_tensor(np.asarray(act, dtype=np.int64), device=full.device)
    return v[a, h0:h0 + Hr].reshape((len(act) * Hr,) + tuple(full.shape[1:])).contiguous()


def _bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))   # bytes: a NaN equals itself


def test_ranking_equals_the_reference_and_stays_inside_its_buffers(st):
    import torch

    from cvxpnpl_amd import _lib, ransac as rn
    from cvxpnpl_amd.api import _ptr

    assert np.array_equal(st.order.cpu().numpy(), np.concatenate(st.order_ref))   # the fixture's ranking, through the wrapper
    L = _lib.ransac_guided_lib()
    stream = C.c_void_p(torch.cuda.current_stream(st.dev).cuda_stream)
    total = int(st.off[-1])
    rs = np.random.RandomState(11)
    pats = [quality_patterns(m, rs) for m in SIZES]
    for name in pats[0]:
        qbuf = torch.full((total + 2 * GUARD,), 123.0, dtype=torch.float64, device=st.dev)
        qbuf[GUARD:GUARD + total] = torch.as_tensor(np.concatenate([p[name] for p in pats]), device=st.dev)
        before = qbuf.clone()
        obuf = torch.full((total + 2 * GUARD,), -9, dtype=torch.int32, device=st.dev)
        q, order = qbuf[GUARD:GUARD + total], obuf[GUARD:GUARD + total]
        assert L.cvxpnpl_ransac_guided_rank(F, _ptr(st.sc.offsets), total, max(SIZES), _ptr(q), _ptr(order), stream) == 0
        torch.cuda.synchronize()
        assert (obuf[:GUARD] == -9).all() and (obuf[GUARD + total:] == -9).all(), name
        assert _bits(qbuf, before), name
        got = order.cpu().numpy()
        for f, m in enumerate(SIZES):
            assert np.array_equal(got[st.off[f]:st.off[f + 1]], rank(pats[f][name])), (name, f, m)
    # max_corr smaller than a scene: the scene is still ranked completely (the stride loop), and nothing else is touched
    obuf = torch.full((total + 2 * GUARD,), -9, dtype=torch.int32, device=st.dev)
    q = torch.as_tensor(np.concatenate(st.q), device=st.dev)
    assert L.cvxpnpl_ransac_guided_rank(F, _ptr(st.sc.offsets), total, 100, _ptr(q), _ptr(obuf[GUARD:GUARD + total]), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(obuf[GUARD:GUARD + total].cpu().numpy(), np.concatenate(st.order_ref))
    assert (obuf[:GUARD] == -9).all() and (obuf[GUARD + total:] == -9).all()
    with pytest.raises(ValueError):
        rn.rank_scenes(st.sc, torch.zeros(total, dtype=torch.float32, device=st.dev))
    with pytest.raises(ValueError):
        rn.rank_scenes(st.sc, torch.zeros(total + 1, dtype=torch.float64, device=st.dev))


@pytest.mark.parametrize("pf", POOLS)
def test_fixed_sampler_equals_the_reference(st, pf):
    import torch

    from cvxpnpl_amd import ransac as rn

    p2, p3, Kh, idx = rn.sample_scenes_guided(st.sc, H_FIX, st.order, pf, want_idx=True)
    assert idx.shape == (F * H_FIX, 4) and idx.dtype == torch.int32 and p2.shape == (F * H_FIX, 4, 2) and p3.shape == (F * H_FIX, 4, 3)
    ref = np.stack([guided_sets(H_FIX, SIZES[f], st.order_ref[f], pf, st.seeds[f]) for f in range(F)])   # [F, H, 4]
    got = idx.cpu().numpy().reshape(F, H_FIX, 4)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert (np.sort(got, axis=-1)[..., 1:] != np.sort(got, axis=-1)[..., :-1]).all()   # four distinct correspondences
    x2 = np.stack([st.xs[f][ref[f]] for f in range(F)]).reshape(F * H_FIX, 4, 2)
    x3 = np.stack([st.Xs[f][ref[f]] for f in range(F)]).reshape(F * H_FIX, 4, 3)
    assert np.array_equal(p2.cpu().numpy(), x2) and np.array_equal(p3.cpu().numpy(), x3)   # the scene's rows at idx
    assert (Kh is None) == (not st.per)
    if st.per:
        assert np.array_equal(Kh.cpu().numpy(), np.repeat(st.K, H_FIX, axis=0))
    for a, b in zip((p2, p3, idx), (st.fix[pf][0], st.fix[pf][1], st.fix[pf][3])):   # a smaller budget is a prefix of a larger one
        assert torch.equal(a, _rows(b, F, range(F), 0, H_FIX))
    if pf == 0:   # the uniform sampler, bit for bit, and the ranking is not read
        u2, u3, uK, ui = rn.sample_scenes(st.sc, H_FIX, want_idx=True)
        assert torch.equal(p2, u2) and torch.equal(p3, u3) and torch.equal(idx, ui) and ((Kh is None and uK is None) or torch.equal(Kh, uK))
        junk = torch.full_like(st.order, 2**31 - 1)
        assert torch.equal(rn.sample_scenes_guided(st.sc, H_FIX, junk, 0, want_idx=True)[3], ui)
    else:         # from pool_full on the draws are the uniform ones
        ui = rn.sample_scenes(st.sc, H_FIX, want_idx=True)[3]
        tail = slice(min(pf, H_FIX), H_FIX)
        assert torch.equal(idx.reshape(F, H_FIX, 4)[:, tail], ui.reshape(F, H_FIX, 4)[:, tail])
        if pf >= H_FIX:
            assert not torch.equal(idx, ui)


@pytest.mark.parametrize("h0", [0, 64, 192])
def test_round_sampler_draws_the_rows_of_the_fixed_guided_sampler(st, h0):
    import torch

    from cvxpnpl_amd import ransac as rn

    lists = {"identity": list(range(F)), "every_other": list(range(0, F, 2)), "one": [F - 3], "reversed": list(range(F - 1, -1, -1))}
    for pf in POOLS:
        f2, f3, fK, fi = st.fix[pf]
        for rh, cap in CFG.values():
            if h0 >= cap:
                continue
            Hr = min(rh, cap - h0)
            for name, act in lists.items():
                a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
                p2, p3, Kh, idx = rn.sample_active_guided(st.sc, a, len(act), h0, Hr, cap, st.order, pf, want_idx=True)
                assert idx.shape == (len(act) * Hr, 4) and p2.shape == (len(act) * Hr, 4, 2) and p3.shape == (len(act) * Hr, 4, 3)
                assert torch.equal(idx, _rows(fi, F, act, h0, Hr)), (pf, name, rh)
                assert torch.equal(p2, _rows(f2, F, act, h0, Hr)) and torch.equal(p3, _rows(f3, F, act, h0, Hr)), (pf, name, rh)
                assert (Kh is None) == (not st.per)
                if st.per:
                    assert torch.equal(Kh, _rows(fK, F, act, h0, Hr)), (pf, name, rh)
    # a longer tensor than n_active: only the first n_active entries count
    a = torch.as_tensor(list(range(F)), dtype=torch.int32, device=st.dev)
    p2, _, _ = rn.sample_active_guided(st.sc, a, 3, h0, 8, 200, st.order, 200)
    assert torch.equal(p2, _rows(st.fix[200][0], F, [0, 1, 2], h0, 8))
    # at pool_full = 0 it is the unguided round sampler
    u = rn.sample_active(st.sc, a, F, h0, 8, 200, want_idx=True)
    g = rn.sample_active_guided(st.sc, a, F, h0, 8, 200, st.order, 0, want_idx=True)
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(u, g))


def test_nothing_active_and_entries_out_of_range(st):
    import torch

    from cvxpnpl_amd import _lib, ransac as rn
    from cvxpnpl_amd.api import _ptr

    sc, pf, cap, Hr, h0 = st.sc, 10**6, 200, 64, 64
    a = torch.arange(F, dtype=torch.int32, device=st.dev)
    p2, p3, Kh, idx = rn.sample_active_guided(sc, a, 0, 0, 64, cap, st.order, pf, want_idx=True)   # n_active = 0: nothing is launched
    assert p2.shape[0] == 0 and p3.shape[0] == 0 and idx.shape[0] == 0
    # entries of active outside [0, F): skipped, not clamped.  Three bad entries around one good one (scene 6).
    bad = torch.tensor([-1, F, 6, 2**31 - 1], dtype=torch.int32, device=st.dev)
    A = 4
    L = _lib.ransac_guided_lib()
    stream = C.c_void_p(torch.cuda.current_stream(st.dev).cuda_stream)
    p2 = torch.full((A * Hr, 4, 2), -7.0, dtype=torch.float64, device=st.dev)
    p3 = torch.full((A * Hr, 4, 3), -7.0, dtype=torch.float64, device=st.dev)
    Kh = torch.full((A * Hr, 3, 3), -7.0, dtype=torch.float64, device=st.dev)
    idx = torch.full((A * Hr, 4), -7, dtype=torch.int32, device=st.dev)
    assert L.cvxpnpl_ransac_guided_sample_active(F, A, _ptr(bad), h0, Hr, cap, pf, _ptr(sc.offsets), sc.total, _ptr(sc.seeds), _ptr(st.order),
                                                 _ptr(sc.x), _ptr(sc.X), _ptr(sc.K) if st.per else None, _ptr(idx), _ptr(p2), _ptr(p3),
                                                 _ptr(Kh) if st.per else None, stream) == 0
    torch.cuda.synchronize()
    good = slice(2 * Hr, 3 * Hr)
    f2, f3, fK, fi = st.fix[pf]
    for buf, ref in ((p2, f2), (p3, f3), (idx, fi)) + (((Kh, fK),) if st.per else ()):
        assert torch.equal(buf[good], _rows(ref, F, [6], h0, Hr))
        assert (torch.cat([buf[:2 * Hr], buf[3 * Hr:]]) == -7).all()
    # entries of order outside [0, M_f): the NaN hypothesis with idx = -1, for exactly the hypotheses that draw such a rank
    f, m = 6, SIZES[6]
    broken = st.order.clone()
    spoiled = {0: -1, 5: m, 40: 2**31 - 1, 77: -2**31}   # rank -> what the ranking holds there
    for r, v in spoiled.items():
        broken[st.off[f] + r] = v
    ranks = guided_sets(H_FIX, m, np.arange(m), pf, st.seeds[f])          # the identity ranking: the ranks every hypothesis draws
    hit = np.isin(ranks, list(spoiled)).any(axis=1)
    assert hit[0] and hit.sum() >= 10 and (~hit).sum() >= 10             # h = 0 draws ranks 0 .. 3
    outs = [rn.sample_scenes_guided(sc, H_FIX, broken, pf, want_idx=True),
            rn.sample_active_guided(sc, a, F, 0, H_FIX, cap, broken, pf, want_idx=True)]
    for p2, p3, Kh, idx in outs:
        for buf, ref in ((p2, f2), (p3, f3), (idx, fi)) + (((Kh, fK),) if st.per else ()):
            others = [g for g in range(F) if g != f]
            assert torch.equal(_rows(buf, F, others, 0, H_FIX), _rows(ref, F, others, 0, H_FIX))   # the other scenes: untouched
        i6, a6, b6 = (_rows(v, F, [f], 0, H_FIX).cpu().numpy() for v in (idx, p2, p3))
        assert (i6[hit] == -1).all() and np.isnan(a6[hit]).all() and np.isnan(b6[hit]).all()
        assert np.array_equal(i6[~hit], _rows(fi, F, [f], 0, H_FIX).cpu().numpy()[~hit])
        assert np.array_equal(a6[~hit], _rows(f2, F, [f], 0, H_FIX).cpu().numpy()[~hit])
        if st.per:
            assert torch.equal(_rows(Kh, F, [f], 0, H_FIX), _rows(fK, F, [f], 0, H_FIX))            # K_hyp is written either way
    for args in ((sc, a, -1, 0, 8, cap, st.order, pf), (sc, a, F, 4, 8, 11, st.order, pf), (sc, a, F, 0, 8, cap, st.order, -1),
                 (sc, a, F, 0, 8, cap, st.order.to(torch.int64), pf), (sc, a, F, 0, 8, cap, st.order[:-1], pf)):
        with pytest.raises(ValueError):
            rn.sample_active_guided(*args)
    with pytest.raises(ValueError):
        rn.sample_scenes_guided(sc, 8, st.order, 1.5)


def test_more_scenes_than_one_grid_dimension_holds():
    """66 000 scenes of 5 correspondences: two slabs of the ranking's and of both samplers' grids."""
    import torch

    from cvxpnpl_amd import ransac as rn

    dev = torch.device("cuda:0")
    nF, m, pf, cap = 66000, 5, 8, 3
    rs = np.random.RandomState(23)
    q = np.round(rs.random_sample((nF, m)), 1)   # one decimal: ties are common
    sc = rn.pack_scenes(rs.random_sample((nF * m, 2)), rs.random_sample((nF * m, 3)), np.eye(3), sizes=[m] * nF, device=dev, seeds=list(range(nF)))
    order = rn.rank_scenes(sc, torch.as_tensor(q.reshape(-1), device=dev))
    ref_order = np.argsort(-q, axis=1, kind="stable")
    assert np.array_equal(order.cpu().numpy().reshape(nF, m), ref_order)
    f2, f3, _, fi = rn.sample_scenes_guided(sc, cap, order, pf, want_idx=True)
    got = fi.cpu().numpy().reshape(nF, cap, 4)
    for f in (0, 463, 65534, 65535, 65999):
        assert np.array_equal(got[f], guided_sets(cap, m, ref_order[f], pf, f)), f
    act = list(range(nF - 1, -1, -1))
    a = torch.as_tensor(act, dtype=torch.int32, device=dev)
    p2, p3, _, idx = rn.sample_active_guided(sc, a, nF, 1, 2, cap, order, pf, want_idx=True)
    assert torch.equal(idx, _rows(fi, nF, act, 1, 2)) and torch.equal(p2, _rows(f2, nF, act, 1, 2)) and torch.equal(p3, _rows(f3, nF, act, 1, 2))


def _reproj(R, t, K, x, X):
    Xc = X @ R.T + t
    uvw = Xc @ K.T
    with np.errstate(all="ignore"):
        return np.linalg.norm(uvw[:, :2] / uvw[:, 2:3] - x, axis=-1)


KEYS = ("R", "t", "inliers", "offsets", "head")


def _same(a, b, keys=KEYS):
    return all(_bits(a[k], b[k]) for k in keys)


def test_whole_call_without_guidance_is_the_call_of_before(st):
    from cvxpnpl_amd import ransac as rn

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    d0 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, **kw)
    d1 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, quality=None, pool_full=None, **kw)
    assert set(d0) == set(d1) and "pool_full" not in d1 and _same(d0, d1)                 # quality=None is the call without the keyword
    d2 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, quality=st.q, pool_full=0, **kw)
    assert set(d2) == set(d0) | {"pool_full"} and d2["pool_full"] == 0 and _same(d0, d2)  # pool_full = 0 is the uniform call
    a0 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, **kw)
    a1 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, quality=None, **kw)
    a2 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, quality=st.q, pool_full=0, **kw)
    for b in (a1, a2):
        assert _same(a0, b, KEYS + ("hyp_used",)) and a0["rounds"] == b["rounds"]
    assert set(a1) == set(a0) and set(a2) == set(a0) | {"pool_full"}


def test_whole_call_guided_is_deterministic_and_takes_every_form_of_quality(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev)
    g0 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, quality=st.q, **kw)
    g1 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, quality=st.q, **kw)
    assert g0["pool_full"] == 128 and _same(g0, g1)                                        # the default pool_full is n_hyp
    assert g0["R"].shape == (F, 3, 3) and g0["inliers"].shape == (sum(SIZES),)
    packed = dict(sizes=SIZES, **kw)
    x, X = np.concatenate(st.xs), np.concatenate(st.Xs)
    qs = {"float64": np.concatenate(st.q), "float32 tensor on the device": torch.as_tensor(np.concatenate(st.q), device=st.dev).float(),
          "list of numbers": [float(np.float32(v)) for v in np.concatenate(st.q)]}
    g32 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=128, quality=[a.astype(np.float32) for a in st.q], **kw)
    for name, q in qs.items():
        g = rn.ransac_pnp_batch(x, X, st.K, n_hyp=128, quality=q, **packed)
        assert _same(g, g0 if name == "float64" else g32), name
    big = [f for f in range(F) if SIZES[f] >= 63]
    assert all(int(g0["n_inliers"][f]) >= 0.3 * SIZES[f] for f in big)                     # at most 0.6 of a scene is clutter
    a0 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, quality=st.q, polish=True, **kw)
    a1 = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, quality=st.q, polish=True, **kw)
    assert _same(a0, a1, KEYS + ("hyp_used",)) and a0["rounds"] == a1["rounds"] and a0["pool_full"] == 200
    assert set(a0) == {"R", "t", "inliers", "offsets", "n_inliers", "status", "n_certified", "best_index", "head", "sizes", "n_hyp", "refine",
                       "hyp_used", "rounds", "confidence", "pool_full"}


def test_whole_call_with_confidence_equals_fixed_guided_calls_at_the_budgets_used(st):
    """Per distinct hyp_used u, the scenes that stopped at u against ransac_pnp_batch(n_hyp=u, quality, the same pool_full): the rules of
    the adaptive whole-call test (masks equal apart from correspondences within 1e-6 px of the threshold, then poses to 1e-8, status and
    best_index equal; at most one scene set aside in all -- the solves run at another batch size and layout)."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    kw = dict(thresh=THRESH, seed=SEED, device=st.dev, quality=st.q, pool_full=200, refit=False)
    out = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=200, confidence=CONF, round_hyp=64, **kw)
    used = out["hyp_used"].numpy()
    assert out["hyp_used"].dtype == torch.int32 and used.shape == (F,) and out["pool_full"] == 200 and out["n_hyp"] == 200
    assert set(used.tolist()) <= {64, 128, 192, 200}
    print("whole call: hyp_used", used.tolist())
    off, inl = st.off, out["inliers"].cpu().numpy()
    Rb, tb = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    aside = []
    for u in sorted(set(used.tolist())):
        one = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=int(u), **kw)
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


def test_guidance_helps_where_the_reference_says_it_should():
    """32 scenes of 100 correspondences, 70 % clutter, sigma 0.5 px, a budget of 32 hypotheses.  From the numpy reference alone: guided
    by an informative quality, at least 90 % of the scenes draw an all-inlier minimal set; uniformly, fewer than half do.  Then every
    scene with a predicted all-inlier guided draw comes back with at least half of its planted inliers."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    nF, M, H, PF, seed0 = 32, 100, 32, 1024, 900   # (seed0: chosen once, on the reference alone)
    rs = np.random.RandomState(seed0)
    scenes = [synth.make_ransac(1, n_corr=M, outlier_frac=0.7, sigma=0.5, seed=seed0 + f) for f in range(nF)]
    qs = [planted_quality(d["inlier"], rs) for d in scenes]
    guided = np.array([first_all_inlier(guided_sets(H, M, rank(qs[f]), PF, SEED + f), scenes[f]["inlier"]) for f in range(nF)])
    uniform = np.array([first_all_inlier(synth.philox_minimal_sets(H, M, 4, SEED + f), scenes[f]["inlier"]) for f in range(nF)])
    print("reference: all-inlier set among the 32, guided", float((guided >= 0).mean()), "at hypothesis 0", float((guided == 0).mean()),
          "uniform", float((uniform >= 0).mean()))
    assert (guided >= 0).mean() >= 0.9 and (uniform >= 0).mean() < 0.5
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    out = rn.ransac_pnp_batch([d["scene_2d"] for d in scenes], [d["scene_3d"] for d in scenes], synth.K_KINECT, n_hyp=H, thresh=THRESH, seed=SEED,
                              quality=qs, pool_full=PF, device=torch.device("cuda:0"))
    inl, off = out["inliers"].cpu().numpy(), out["offsets"].cpu().numpy()
    kept = np.array([(inl[off[f]:off[f + 1]] & scenes[f]["inlier"]).sum() for f in range(nF)])
    planted = np.array([d["inlier"].sum() for d in scenes])
    print("planted inliers kept per scene", kept.tolist(), "of", planted.tolist())
    for f in np.nonzero(guided >= 0)[0]:
        assert 2 * kept[f] >= planted[f], (f, kept[f], planted[f])
