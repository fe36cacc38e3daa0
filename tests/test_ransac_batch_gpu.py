"""RANSAC over many scenes of different sizes (cvxpnpl_amd.ransac.ransac_pnp_batch, libcvxpnpl_amd_ransac.so).

Every stage is held against the existing single-scene kernel on the same inputs (sample_minimal_sets, score_hypotheses, select_best,
assemble_subsets, refit_update: the solver library, which this feature does not touch), then the whole call against ransac_pnp per scene.
48 scenes of 4 .. 700 correspondences (exactly 4, sizes that are no multiple of 64, sizes above one scoring tile of 512), outlier
fractions 0 .. 0.5, sigma 0.5 px, 512 hypotheses per scene; once with a shared K and once with a K per scene."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, H, THRESH, SEED = 48, 512, 2.0, 1000
SIZES = [int(round(v)) for v in np.geomspace(4, 700, F)]
assert SIZES[0] == 4 and SIZES[-1] == 700 and any(s > 512 for s in SIZES) and any(s % 64 for s in SIZES)


def _make_scenes(per_scene_K, sizes=SIZES, seed0=100):
    from cvxpnpl_amd import synth

    xs, Xs, Ks = [], [], []
    n = len(sizes)
    for f, m in enumerate(sizes):
        K = np.array(synth.K_KINECT)
        if per_scene_K:
            K[0, 0] *= 0.8 + 0.4 * f / max(n - 1, 1)
            K[1, 1] *= 0.8 + 0.4 * f / max(n - 1, 1)
        frac = 0.5 * ((7 * f) % n) / max(n - 1, 1)
        d = synth.make_ransac(1, n_corr=m, outlier_frac=frac, sigma=0.5, seed=seed0 + f, K=K)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); Ks.append(K)
    return xs, Xs, (np.stack(Ks) if per_scene_K else Ks[0])


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """The stages of one frame set, computed once per K mode: scenes, minimal sets, the F * H solves, counts and the selection."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_lib()
    s = _State()
    s.dev = torch.device("cuda:0")
    s.per = request.param == "per_scene_K"
    s.xs, s.Xs, s.K = _make_scenes(s.per)
    s.sc = rn.pack_scenes(s.xs, s.Xs, s.K, device=s.dev)
    s.seeds = [SEED + f for f in range(F)]
    s.x = [torch.as_tensor(a, device=s.dev) for a in s.xs]
    s.X = [torch.as_tensor(a, device=s.dev) for a in s.Xs]
    s.Kf = [torch.as_tensor(s.K[f] if s.per else s.K, device=s.dev) for f in range(F)]
    s.off = np.concatenate([[0], np.cumsum(SIZES)])
    s.p2, s.p3, s.Kh, s.idx = rn.sample_scenes(s.sc, H, s.seeds, want_idx=True)
    s.res = ca.pnp_batch(s.p2, s.p3, s.Kh if s.per else s.sc.K, eps=1e-6, max_iters=100)
    s.count = rn.score_scenes(s.sc, s.res.R, s.res.t, THRESH, status=s.res.status, usable=(0, 2))
    s.sel = rn.select_scenes(s.sc, s.count, s.res.R, s.res.t, s.res.status, THRESH)
    torch.cuda.synchronize()
    return s


def _seg(t, f):
    return t[f * H:(f + 1) * H]


def _reproj(R, t, K, x, X):
    """float64 numpy: reprojection error [.., M] in pixels and depth [.., M] of the scene under pose(s) R [..,3,3], t [..,3]"""
    Xc = np.einsum("...ij,mj->...mi", R, X) + t[..., None, :]
    uvw = np.einsum("ij,...mj->...mi", K, Xc)
    with np.errstate(all="ignore"):
        err = np.linalg.norm(uvw[..., :2] / uvw[..., 2:3] - x, axis=-1)
    return err, Xc[..., 2]


def test_sampler_draws_what_the_single_scene_sampler_draws(st):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import synth

    assert st.idx.shape == (F * H, 4) and st.p2.shape == (F * H, 4, 2) and st.p3.shape == (F * H, 4, 3)
    for f in range(F):
        p2, p3, idx = ca.sample_minimal_sets(st.x[f], st.X[f], H, 4, st.seeds[f], want_idx=True)
        mine = _seg(st.idx, f)
        assert torch.equal(mine, idx), f
        assert np.array_equal(mine.cpu().numpy(), synth.philox_minimal_sets(H, SIZES[f], 4, st.seeds[f])), f
        assert torch.equal(_seg(st.p2, f), st.x[f][mine.long()]) and torch.equal(_seg(st.p3, f), st.X[f][mine.long()]), f
        assert torch.equal(_seg(st.p2, f), p2) and torch.equal(_seg(st.p3, f), p3), f
        if st.per:
            assert torch.equal(_seg(st.Kh, f), st.Kf[f].expand(H, 3, 3)), f
    assert (st.Kh is None) == (not st.per)


def _score_differences(sc_sizes, count, res, x, X, Kf, scenes, n_hyp):
    """count of the scenes kernel against cvxpnpl_score_hypotheses, scene by scene; a difference is admissible only where float64 numpy
    puts the reprojection error within 1e-9 px of the threshold or the depth within 1e-12 of 0.  Returns (differing pairs, all pairs)."""
    import cvxpnpl_amd as ca

    differing, pairs = 0, 0
    for f in scenes:
        sl = slice(f * n_hyp, (f + 1) * n_hyp)
        ref = ca.score_hypotheses(res.R[sl], res.t[sl], Kf[f], x[f], X[f], THRESH, status=res.status[sl], usable=(0, 2))
        mine = count[sl]
        pairs += n_hyp * sc_sizes[f]
        bad = (ref != mine).nonzero().flatten().cpu().numpy()
        for h in bad:
            err, depth = _reproj(res.R[sl][h].cpu().numpy(), res.t[sl][h].cpu().numpy(), Kf[f].cpu().numpy(), x[f].cpu().numpy(), X[f].cpu().numpy())
            border = int(((np.abs(err - THRESH) < 1e-9) | (np.abs(depth) < 1e-12)).sum())
            d = abs(int(ref[h]) - int(mine[h]))
            assert d <= border, f"scene {f} hypothesis {h}: counts {int(ref[h])} / {int(mine[h])} with {border} borderline correspondences"
            differing += d
    return differing, pairs


def test_scoring_equals_the_single_scene_kernel(st):
    differing, pairs = _score_differences(SIZES, st.count, st.res, st.x, st.X, st.Kf, range(F), H)
    print(f"scoring: {differing} differing (hypothesis, correspondence) pairs of {pairs}")
    assert differing <= 1e-6 * pairs, (differing, pairs)


def _select_ref(st, f, count, res):
    import cvxpnpl_amd as ca

    sl = slice(f * H, (f + 1) * H)
    return ca.select_best(count[sl], res.R[sl], res.t[sl], res.status[sl], st.Kf[f], st.x[f], st.X[f], THRESH)


def test_selection_equals_select_best_per_scene(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    R, t, head, mask = st.sel
    for f in range(F):
        R1, t1, h1, m1 = _select_ref(st, f, st.count, st.res)
        assert torch.equal(head[f], h1) and torch.equal(R[f], R1[0]) and torch.equal(t[f], t1[0]), f
        assert torch.equal(mask[st.off[f]:st.off[f + 1]], m1[0]), f
    # all counts equal: the lowest index wins in every scene
    flat = torch.full_like(st.count, 3)
    R, t, head, mask = rn.select_scenes(st.sc, flat, st.res.R, st.res.t, st.res.status, THRESH)
    assert (head[:, 2] == 0).all()
    for f in range(F):
        R1, t1, h1, m1 = _select_ref(st, f, flat, st.res)
        assert torch.equal(head[f], h1) and torch.equal(R[f], R1[0]) and torch.equal(t[f], t1[0]), f
        assert torch.equal(mask[st.off[f]:st.off[f + 1]], m1[0]), f


def _assembly_against_subsets(st, mask):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    Bt, Qt, cnt = rn.assemble_consensus(st.sc, mask)
    nan = []
    for f in range(F):
        mk = mask[st.off[f]:st.off[f + 1]]
        Bs, Qs, cs = ca.assemble_subsets(st.x[f], st.X[f], st.Kf[f], mk[None])
        assert int(cnt[f]) == int(cs[0]) == int(mk.ne(0).sum()), f
        if torch.isnan(Qs).any():
            assert torch.isnan(Bt[f]).all() and torch.isnan(Qt[f]).all(), f
            nan.append(f)
            continue
        # the tolerance of test_subset_assembly_equals_the_assembly_of_the_gathered_subset (the summation order differs: no bit-equality)
        assert float((Qt[f] - Qs[0]).abs().max()) <= 1e-11 * float(Qs.abs().max()), f
        assert float((Bt[f] - Bs[0]).abs().max()) <= 1e-9 * max(1.0, float(Bs.abs().max())), f
    return Bt, Qt, cnt, nan


def test_consensus_assembly_equals_assemble_subsets_per_scene(st):
    import torch

    _, _, _, nan = _assembly_against_subsets(st, st.sel[3])  # the consensus sets of the selection
    assert all(SIZES[f] < 16 for f in nan), nan
    # random subsets, one scene cut down to two correspondences: NaN for that scene only
    rs = np.random.RandomState(3)
    m = (rs.rand(int(st.off[-1])) < 0.5).astype(np.uint8)
    j = F - 5
    m[st.off[j]:st.off[j + 1]] = 0
    m[st.off[j] + 3] = m[st.off[j + 1] - 1] = 1
    Bt, Qt, cnt, nan = _assembly_against_subsets(st, torch.as_tensor(m, device=st.dev))
    assert j in nan and int(cnt[j]) == 2
    assert torch.isfinite(Qt[j - 1]).all() and torch.isfinite(Qt[j + 1]).all() and torch.isfinite(Bt[j + 1]).all()
    assert all(f == j or SIZES[f] < 16 for f in nan), nan


def test_refit_update_equals_refit_update_per_scene(st):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    R, t, head, mask = (a.clone() for a in st.sel)
    Bt, Qt, cnt = rn.assemble_consensus(st.sc, mask)
    fit = ca.solve_cost_batch(Qt, Bt)
    j = F - 3   # a large scene whose refit would be taken: given a deliberately unusable fit, it keeps pose, mask and head
    assert int(fit.status[j]) in (0, 2) and int(cnt[j]) >= 4
    fit.status[j] = 3
    before = (R.clone(), t.clone(), head.clone(), mask.clone())
    rn.refit_update_scenes(st.sc, fit, cnt, THRESH, R, t, head, mask)
    taken = 0
    for f in range(F):
        R1, t1, h1, m1 = _select_ref(st, f, st.count, st.res)
        one = ca.BatchResult(R=fit.R[f:f + 1].clone(), t=fit.t[f:f + 1].clone(), status=fit.status[f:f + 1].clone())
        ca.refit_update(one, cnt[f:f + 1].clone(), st.Kf[f], st.x[f], st.X[f], THRESH, R1, t1, h1, m1)
        assert torch.equal(head[f], h1) and torch.equal(R[f], R1[0]) and torch.equal(t[f], t1[0]), f
        assert torch.equal(mask[st.off[f]:st.off[f + 1]], m1[0]), f
        taken += int(not torch.equal(R[f], before[0][f]))
    assert taken >= 1, taken   # (the rule is exercised both ways)
    assert torch.equal(R[j], before[0][j]) and torch.equal(t[j], before[1][j]) and torch.equal(head[j], before[2][j])
    assert torch.equal(mask[st.off[j]:st.off[j + 1]], before[3][st.off[j]:st.off[j + 1]])


def _against_single_scene(out, xs, Xs, K, per, seeds, n_hyp):
    """The rules of the whole-call comparison: per scene against ransac_pnp.  Returns (borderline correspondences per scene, scenes set
    aside because a borderline correspondence changed the winner)."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    off = out["offsets"].cpu().numpy()
    inl = out["inliers"].cpu().numpy()
    Rb, tb = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    borderline, aside = [], []
    for f in range(len(xs)):
        Kf = K[f] if per else K
        one = rn.ransac_pnp(xs[f], Xs[f], Kf, seed=seeds[f], n_hyp=n_hyp, thresh=THRESH)
        R1, t1, m1 = one["R"].cpu().numpy(), one["t"].cpu().numpy(), one["inliers"].cpu().numpy()
        err, _ = _reproj(R1, t1, Kf, xs[f], Xs[f])
        border = np.abs(err - THRESH) < 1e-6
        b = int(border.sum())
        borderline.append(b)
        mb = inl[off[f]:off[f + 1]]
        if ((mb != m1) & ~border).any():   # the masks differ beyond the borderline correspondences
            aside.append(f)
            assert int(out["n_inliers"][f]) >= one["n_inliers"] - b, (f, int(out["n_inliers"][f]), one["n_inliers"], b)
            continue
        assert abs(int(out["n_inliers"][f]) - one["n_inliers"]) <= b, f
        assert int(out["n_inliers"][f]) == int(mb.sum()), f
        if np.array_equal(mb, m1):
            if not (np.isfinite(R1).all() and np.isfinite(t1).all()):   # no usable pose in this scene: the same non-finite entries
                assert np.array_equal(np.isfinite(Rb[f]), np.isfinite(R1)) and np.array_equal(np.isfinite(tb[f]), np.isfinite(t1)), f
                continue
            geo = float(synth.geodesic(Rb[f], R1))
            rel = float(np.abs(tb[f] - t1).max() / max(np.abs(t1).max(), 1e-300))
            assert geo <= 1e-8 and rel <= 1e-8, (f, geo, rel)
            assert int(out["status"][f]) == one["status"], f
    return borderline, aside


def test_whole_call_equals_ransac_pnp_per_scene(st):
    """Recorded on the MI355X: see DESIGN.md section 13 (borderline correspondences and scenes set aside are printed)."""
    from cvxpnpl_amd import ransac as rn

    out = rn.ransac_pnp_batch(st.xs, st.Xs, st.K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev)
    assert out["R"].shape == (F, 3, 3) and out["t"].shape == (F, 3) and out["inliers"].shape == (sum(SIZES),) and out["offsets"].shape == (F + 1,)
    assert all(out[k].shape == (F,) for k in ("n_inliers", "status", "n_certified", "best_index"))
    borderline, aside = _against_single_scene(out, st.xs, st.Xs, st.K, st.per, st.seeds, H)
    print(f"whole call: {sum(borderline)} borderline correspondences in {sum(b > 0 for b in borderline)} scenes, set aside: {aside}")
    assert len(aside) <= 1, aside
    # the packed form gives the same call
    import torch

    packed = rn.ransac_pnp_batch(np.concatenate(st.xs), np.concatenate(st.Xs), st.K, n_hyp=H, thresh=THRESH, seed=st.seeds, sizes=SIZES, device=st.dev)
    assert torch.equal(packed["R"], out["R"]) and torch.equal(packed["inliers"], out["inliers"]) and torch.equal(packed["head"], out["head"])


def test_one_scene_determinism_and_streams(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    f = F - 2
    one = rn.ransac_pnp_batch([st.xs[f]], [st.Xs[f]], st.K[f] if st.per else st.K, n_hyp=H, thresh=THRESH, seed=77, device=st.dev)
    _, aside = _against_single_scene(one, [st.xs[f]], [st.Xs[f]], st.K[f:f + 1] if st.per else st.K, st.per, [77], H)
    assert not aside

    def call(n):
        return rn.ransac_pnp_batch(st.xs[:n], st.Xs[:n], st.K[:n] if st.per else st.K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev)

    def same(a, b):
        return all(torch.equal(a[k], b[k]) for k in ("R", "t", "inliers", "offsets", "head"))

    a, b = call(F), call(F)
    assert same(a, b)   # two identical calls are bit-identical
    c = call(5)
    side = torch.cuda.Stream(device=st.dev)
    side.wait_stream(torch.cuda.current_stream(st.dev))
    with torch.cuda.stream(side):   # a call on a side stream directly followed by one of a different F
        a2 = call(F)
        c2 = call(5)
    side.synchronize()
    assert same(a, a2) and same(c, c2)


def test_more_hypotheses_than_one_grid_dimension_holds():
    """F = 300 scenes x 4096 hypotheses = 1 228 800 problems (4 800 workgroups of 256 lanes over a two-dimensional grid; the solve sees more
    than 65 535 wavefronts): completes, and the counts agree with the single-scene kernel on a sample of scenes."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    dev = torch.device("cuda:0")
    nF, nH = 300, 4096
    sizes = [SIZES[(5 * f) % F] for f in range(nF)]
    xs, Xs, K = _make_scenes(False, sizes=sizes, seed0=4000)
    sc = rn.pack_scenes(xs, Xs, K, device=dev)
    p2, p3, Kh = rn.sample_scenes(sc, nH, list(range(nF)))
    res = ca.pnp_batch(p2, p3, sc.K, eps=1e-6, max_iters=100)
    count = rn.score_scenes(sc, res.R, res.t, THRESH, status=res.status, usable=(0, 2))
    x = [torch.as_tensor(a, device=dev) for a in xs]
    X = [torch.as_tensor(a, device=dev) for a in Xs]
    sample = [0, 1, 57, 149, 150, 298, 299]

    differing, pairs = _score_differences(sizes, count, res, x, X, [sc.K] * nF, sample, nH)
    assert differing <= 1e-6 * pairs, (differing, pairs)
    out = rn.ransac_pnp_batch(xs, Xs, K, n_hyp=nH, thresh=THRESH, seed=0, device=dev)
    assert out["head"].shape == (nF, 4) and int(out["n_inliers"].min()) >= 0
    big = [f for f in range(nF) if sizes[f] >= 64]
    assert all(int(out["n_inliers"][f]) >= 0.3 * sizes[f] for f in big)   # at most half of a scene is clutter: a consensus was found
    assert (out["best_index"] >= 0).all() and (out["best_index"] < nH).all()
