"""RANSAC over points and lines, many scenes (cvxpnpl_amd.ransac.ransac_pnpl_batch, libcvxpnpl_amd_ransac_pnpl.so).

Every stage is held against something that does not share its code: the draw against the numpy Philox restatement and the point-only
sampler, the minimal and consensus assemblies against assemble_batch on the gathered sets and the CPU oracle, the solves against
pnpl_batch, the scores and masks against float64 numpy restatements of both predicates, selection and the refit rule against numpy; then
the whole call against the stages, against itself and, on point-only scenes, against ransac_pnp_batch.
24 scenes x 256 hypotheses, sigma 0.5 px, outlier shares 0 .. 0.5; once with a shared K and once with a K per scene."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, THRESH, SEED = 256, 2.0, 2000
# (P_f, L_f): one minimal set of each mix, lines only / points only, sizes that are no multiple of 64, one P_f above a point tile of the
# scoring kernel (512) and one L_f above a line tile (256)
SHAPES = [(4, 0), (0, 4), (3, 1), (1, 3), (2, 2), (0, 70), (70, 0), (600, 10), (10, 300), (33, 17), (65, 63), (100, 50), (5, 1), (1, 5), (7, 0),
          (0, 9), (129, 31), (20, 20), (64, 64), (250, 3), (3, 90), (47, 0), (0, 130), (12, 13)]
F = len(SHAPES)
SMALL = [0, 1, 2, 3, 4]   # every hypothesis of these is compared in the assembly and solve tests, 64 of every other scene
assert F == 24 and any(p > 512 for p, _ in SHAPES) and any(l > 256 for _, l in SHAPES)


def _make_scenes(per_scene_K, shapes=SHAPES, seed0=300, sigma=0.5, max_frac=0.5):
    from cvxpnpl_amd import synth

    out, Ks, n = [], [], len(shapes)
    for f, (p, l) in enumerate(shapes):
        K = np.array(synth.K_KINECT)
        if per_scene_K:
            K[0, 0] *= 0.8 + 0.4 * f / max(n - 1, 1)
            K[1, 1] *= 0.8 + 0.4 * f / max(n - 1, 1)
        frac = max_frac * ((7 * f) % n) / max(n - 1, 1) if p + l > 8 else 0.0
        out.append(synth.make_ransac_pnpl(p, l, outlier_frac=frac, sigma=sigma, seed=seed0 + f, K=K))
        Ks.append(K)
    return out, (np.stack(Ks) if per_scene_K else Ks[0])


def _lists(scenes):
    return [d["pts_2d"] for d in scenes], [d["line_2d"] for d in scenes], [d["pts_3d"] for d in scenes], [d["line_3d"] for d in scenes]


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """The stages of one frame set, computed once per K mode and left unchanged by the tests."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_pnpl_lib()
    s = _State()
    s.dev = torch.device("cuda:0")
    s.per = request.param == "per_scene_K"
    s.scenes, s.K = _make_scenes(s.per)
    s.args = _lists(s.scenes)
    s.seeds = [SEED + f for f in range(F)]
    s.sc = rn.pack_pnpl_scenes(*s.args, s.K, device=s.dev, seeds=s.seeds)
    s.Kf = [s.K[f] if s.per else s.K for f in range(F)]
    s.offp = np.concatenate([[0], np.cumsum([p for p, _ in SHAPES])])
    s.offl = np.concatenate([[0], np.cumsum([l for _, l in SHAPES])])
    s.Q, s.B, s.idx = rn.sample_assemble_scenes(s.sc, H, want_idx=True)
    s.res = rn.solve_minimal_costs(s.Q, s.B, eps=1e-6, max_iters=100)   # (as ransac_pnpl_batch solves them)
    s.count = rn.score_pnpl_scenes(s.sc, s.res.R, s.res.t, THRESH, status=s.res.status, usable=(0, 2))
    s.sel = rn.select_pnpl_scenes(s.sc, s.count, s.res.R, s.res.t, s.res.status, THRESH)
    torch.cuda.synchronize()
    s.R, s.t, s.status = s.res.R.cpu().numpy(), s.res.t.cpu().numpy(), s.res.status.cpu().numpy()
    return s


def _seg(a, f):
    return a[f * H:(f + 1) * H]


# ---- float64 numpy restatements of the two predicates -------------------------------------------------------------------------------------
def _project(R, t, K, X):
    """pixels [.., M, 2] and depth [.., M] of X [M,3] under pose(s) R [..,3,3], t [..,3]"""
    Xc = np.einsum("...ij,mj->...mi", R, X) + t[..., None, :]
    uvw = np.einsum("ij,...mj->...mi", K, Xc)
    with np.errstate(all="ignore"):
        return uvw[..., :2] / uvw[..., 2:3], Xc[..., 2]


def _point_pred(R, t, K, d, thresh=THRESH):
    """(inlier [.., P], borderline [.., P]) of the scene's points"""
    if len(d["pts_3d"]) == 0:
        z = np.zeros(R.shape[:-2] + (0,), bool)
        return z, z
    uv, depth = _project(R, t, K, d["pts_3d"])
    with np.errstate(all="ignore"):
        err = np.linalg.norm(uv - d["pts_2d"], axis=-1)
        return (depth > 0) & (err < thresh), (np.abs(err - thresh) < 1e-9) | (np.abs(depth) < 1e-12)


def _line_pred(R, t, K, d, thresh=THRESH):
    """(inlier [.., L], borderline [.., L]) of the scene's lines: l = (a, 1) x (b, 1); both end points in front of the camera and within
    thresh pixels of l"""
    L = len(d["line_3d"])
    if L == 0:
        z = np.zeros(R.shape[:-2] + (0,), bool)
        return z, z
    a, b = d["line_2d"][:, 0], d["line_2d"][:, 1]
    l = np.cross(np.concatenate([a, np.ones((L, 1))], 1), np.concatenate([b, np.ones((L, 1))], 1))   # [L,3]
    uv, depth = _project(R, t, K, d["line_3d"].reshape(-1, 3))
    uv, depth = uv.reshape(uv.shape[:-2] + (L, 2, 2)), depth.reshape(depth.shape[:-1] + (L, 2))
    with np.errstate(all="ignore"):
        dist = np.abs(uv[..., 0] * l[:, None, 0] + uv[..., 1] * l[:, None, 1] + l[:, None, 2]) / np.hypot(l[:, 0], l[:, 1])[:, None]
        ok = ((depth > 0) & (dist < thresh)).all(-1)
        border = ((np.abs(dist - thresh) < 1e-9) | (np.abs(depth) < 1e-12)).any(-1)
    return ok, border


def _check_masks(st, f, R, t, mp, ml, what):
    """the masks of scene f equal the numpy predicates of the pose, except on borderline correspondences; returns the differing count"""
    d = st.scenes[f]
    ip, bp = _point_pred(R, t, st.Kf[f], d)
    il, bl = _line_pred(R, t, st.Kf[f], d)
    mp, ml = mp[st.offp[f]:st.offp[f + 1]].astype(bool), ml[st.offl[f]:st.offl[f + 1]].astype(bool)
    assert not ((mp != ip) & ~bp).any() and not ((ml != il) & ~bl).any(), (what, f)
    return int((mp != ip).sum() + (ml != il).sum())


# ---- 1. the draw --------------------------------------------------------------------------------------------------------------------------
def test_draw_is_the_philox_draw_over_the_union(st):
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    idx = st.idx.cpu().numpy()
    assert idx.shape == (F * H, 4)
    for f, (p, l) in enumerate(SHAPES):
        assert np.array_equal(_seg(idx, f), synth.philox_minimal_sets(H, p + l, 4, st.seeds[f])), f
    only = [f for f, (p, l) in enumerate(SHAPES) if l == 0]
    assert len(only) >= 3
    sc = rn.pack_scenes([st.args[0][f] for f in only], [st.args[2][f] for f in only], st.K[only] if st.per else st.K, device=st.dev)
    ref = rn.sample_scenes(sc, H, [st.seeds[f] for f in only], want_idx=True)[3]
    for i, f in enumerate(only):
        assert torch.equal(_seg(st.idx, f), _seg(ref, i)), f


# ---- 2. minimal assembly ------------------------------------------------------------------------------------------------------------------
def _gathered(st, f, hyps):
    """the sets of scene f's hypotheses `hyps`, grouped by shape: {k_p: (rows, p2 [n,k_p,2], l2 [n,k_l,2,2], p3, l3)}, each set ordered
    points in draw order, then lines in draw order"""
    d, P = st.scenes[f], SHAPES[f][0]
    idx = _seg(st.idx.cpu().numpy(), f)[hyps]
    srt = np.take_along_axis(idx, np.argsort(idx >= P, axis=1, kind="stable"), 1)
    kp = (idx < P).sum(1)
    out = {}
    for k in np.unique(kp):
        rows = np.nonzero(kp == k)[0]
        ip, il = srt[rows][:, :k], srt[rows][:, k:] - P
        out[int(k)] = (rows, d["pts_2d"][ip], d["line_2d"][il], d["pts_3d"][ip], d["line_3d"][il])
    return out


def _hyps(f):
    return np.arange(H) if f in SMALL else np.arange(0, H, H // 64)


def _oracle_cost(p2, l2, p3, l3, K):
    """(B [27], Q [45], cond(N^T N)) of one set by the CPU oracle: point / line constraints, elimination, A^T A"""
    import oracle
    from cvxpnpl_amd import pack_cost

    Cs, Ns = [], []
    if len(p3):
        Cm, N = oracle.point_constraints(p2, p3, K)
        Cs += list(Cm); Ns += list(N)
    if len(l3):
        Cm, N = oracle.line_constraints(l2, l3, K)
        Cs.append(Cm); Ns.append(N)
    Cm, N = np.concatenate(Cs), np.concatenate(Ns)
    B, A = oracle.eliminate(Cm, N)
    return B.reshape(27), pack_cost(A.T @ A), np.linalg.cond(N.T @ N)


def test_minimal_assembly_equals_assemble_batch_and_the_oracle(st):
    """Bound against assemble_batch: |dQ| <= 1e-11 max|Q|, |dB| <= 1e-9 max(1, max|B|) per set (tests/test_device_toolkit.py).

    Against the oracle, on EVERY compared set, B (its [3,9] is the B27 layout) and Q: |dB| <= 1e-13 cond(N^T N) max(1, max|B|) and
    |dQ| <= 1e-13 cond(N^T N) max|Q|.  Where the figure comes from: both sides solve the 3 x 3 normal equations N^T N B = N^T C in
    float64, unit roundoff u = 2^-53 = 1.1e-16, and the forward error of such a solve is c u cond(N^T N) relative, c a small multiple of
    the lengths of the sums behind it.  A minimal set has at most 12 rows, so N^T N and N^T C are sums of at most 12 products (12 u each),
    the solve of order 3 adds about 3 * 9 u: some 50 u per side, 100 u for the difference of two sides, and a factor sqrt(27) ~ 5 between
    the norm-wise statement of the theory and the largest of 27 entries taken here: 500 u = 5.6e-14, rounded up to 1e-13.  Q = A^T A with
    A = C - N B inherits B's relative error twice over and is held by the same figure.  The bound is that of two correct float64
    eliminations of different order (the oracle eliminates without a centre shift), not a fit to either.  Measured on the MI355X: see
    DESIGN.md section 14."""
    import torch

    import cvxpnpl_amd as ca

    Q, B = st.Q.cpu().numpy(), st.B.cpu().numpy()
    worst_q = worst_b = worst_oq = worst_ob = spread_q = spread_b = 0.0
    n_sets = n_oracle = 0
    for f in range(F):
        hyps = _hyps(f)
        for k, (rows, p2, l2, p3, l3) in _gathered(st, f, hyps).items():
            g = f * H + hyps[rows]
            Bs, Qs = ca.assemble_batch(p2 if k else None, l2 if k < 4 else None, p3 if k else None, l3 if k < 4 else None, st.Kf[f], device=st.dev,
                                       blocked=False)
            Bs, Qs = Bs.cpu().numpy(), Qs.cpu().numpy()
            fin = np.isfinite(Qs).all(1)
            assert np.array_equal(np.isfinite(Q[g]).all(1), fin) and np.array_equal(np.isfinite(B[g]).all(1), fin), (f, k)
            eq = np.abs(Q[g] - Qs).max(1) / np.abs(Qs).max(1)
            eb = np.abs(B[g] - Bs).max(1) / np.maximum(1.0, np.abs(Bs).max(1))
            worst_q, worst_b = max(worst_q, float(eq[fin].max(initial=0))), max(worst_b, float(eb[fin].max(initial=0)))
            n_sets += len(rows)
            for i in np.nonzero(fin)[0]:   # the oracle, on every set that has a cost
                Bo, Qo, cond = _oracle_cost(p2[i], l2[i], p3[i], l3[i], st.Kf[f])
                sq, sb = np.abs(Qo).max() * max(cond, 1.0), max(1.0, np.abs(Bo).max()) * max(cond, 1.0)
                worst_oq = max(worst_oq, float(np.abs(Q[g[i]] - Qo).max() / sq))
                worst_ob = max(worst_ob, float(np.abs(B[g[i]] - Bo).max() / sb))
                spread_q = max(spread_q, float(np.abs(Qs[i] - Qo).max() / sq))
                spread_b = max(spread_b, float(np.abs(Bs[i] - Bo).max() / sb))
                n_oracle += 1
    print(f"minimal assembly, {n_sets} sets: max |dQ| / max|Q| = {worst_q:.3e}, max |dB| / max(1, |B|) = {worst_b:.3e} against assemble_batch; "
          f"against the oracle on {n_oracle} sets, over cond(N^T N): Q {worst_oq:.3e}, B {worst_ob:.3e} (assemble_batch itself: Q {spread_q:.3e}, "
          f"B {spread_b:.3e})")
    assert worst_q <= 1e-11 and worst_b <= 1e-9, (worst_q, worst_b)
    assert worst_oq <= 1e-13 and worst_ob <= 1e-13, (worst_oq, worst_ob)


def test_minimal_assembly_reports_what_it_cannot_assemble(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    # a scene forced below four correspondences through the stage function (the public call refuses it): NaN cost and index -1
    sc, j = st.sc, 9
    off = sc.offsets.clone()
    off[j + 1:] -= SHAPES[j][0] - 2                     # scene j keeps 2 of its points ...
    loff = sc.line_offsets.clone()
    loff[j + 1:] -= SHAPES[j][1] - 1                    # ... and 1 of its lines; the scenes behind it move up in the packed arrays
    keep_p = torch.ones(sc.total, dtype=torch.bool, device=st.dev); keep_p[st.offp[j] + 2:st.offp[j + 1]] = False
    keep_l = torch.ones(sc.line_total, dtype=torch.bool, device=st.dev); keep_l[st.offl[j] + 1:st.offl[j + 1]] = False
    sizes, lsizes = list(sc.sizes), list(sc.line_sizes)
    sizes[j], lsizes[j] = 2, 1
    cut = rn.PnplScenes(sc.x[keep_p].contiguous(), sc.X[keep_p].contiguous(), sc.l2[keep_l].contiguous(), sc.l3[keep_l].contiguous(), off, loff, sizes,
                        lsizes, sc.K, sc.seeds)
    Q, B, idx = rn.sample_assemble_scenes(cut, H, want_idx=True)
    assert torch.isnan(_seg(Q, j)).all() and torch.isnan(_seg(B, j)).all() and (_seg(idx, j) == -1).all()
    for f in (j - 1, j + 1, F - 1):                     # the neighbours are what they were
        assert torch.equal(_seg(Q, f), _seg(st.Q, f)) and torch.equal(_seg(B, f), _seg(st.B, f)) and torch.equal(_seg(idx, f), _seg(st.idx, f)), f
    # a singular K: NaN cost and index -1 (of that scene only, where K is per scene)
    Ks = sc.K.clone()
    if st.per:
        Ks[j, 2, 2] = 0.0
    else:
        Ks[2, 2] = 0.0
    sing = rn.PnplScenes(sc.x, sc.X, sc.l2, sc.l3, sc.offsets, sc.line_offsets, sc.sizes, sc.line_sizes, Ks, sc.seeds)
    Q, B, idx = rn.sample_assemble_scenes(sing, H, want_idx=True)
    assert torch.isnan(_seg(Q, j)).all() and torch.isnan(_seg(B, j)).all() and (_seg(idx, j) == -1).all()
    if st.per:
        for f in (j - 1, j + 1):
            assert torch.equal(_seg(Q, f), _seg(st.Q, f)) and torch.equal(_seg(B, f), _seg(st.B, f)) and torch.equal(_seg(idx, f), _seg(st.idx, f)), f
    else:
        assert torch.isnan(Q).all() and torch.isnan(B).all() and (idx == -1).all()


# ---- 3. the solves ------------------------------------------------------------------------------------------------------------------------
def test_solves_at_the_cost_seam_equal_pnpl_batch_on_the_gathered_sets(st):
    import cvxpnpl_amd as ca
    from cvxpnpl_amd import synth

    worst, n_cert, n_all, differ = 0.0, 0, 0, []
    for f in range(F):
        hyps = _hyps(f)
        for k, (rows, p2, l2, p3, l3) in _gathered(st, f, hyps).items():
            g = f * H + hyps[rows]
            ref = ca.pnpl_batch(p2 if k else None, l2 if k < 4 else None, p3 if k else None, l3 if k < 4 else None, st.Kf[f], eps=1e-6, max_iters=100,
                                device=st.dev)
            rs = ref.status.cpu().numpy()
            bad = np.nonzero(st.status[g] != rs)[0]
            if len(bad):
                differ.append((f, k, len(bad), len(rows), np.bincount(st.status[g][bad], minlength=5).tolist(), np.bincount(rs[bad], minlength=5).tolist()))
            cert = (rs == 0) & (st.status[g] == 0)
            n_cert += int(cert.sum()); n_all += len(rows)
            if cert.any():
                worst = max(worst, float(synth.geodesic(st.R[g][cert], ref.R.cpu().numpy()[cert]).max()))
    print(f"solves: {n_cert} certified by both of {n_all}, max geodesic between the two entries {worst:.3e} rad; statuses differ in "
          f"{sum(d[2] for d in differ)} sets: (scene, points in the set, differing, sets, seam statuses, pnpl_batch statuses) {differ}")
    assert not differ, differ
    assert worst <= 1e-8, worst


# ---- 4. scores ----------------------------------------------------------------------------------------------------------------------------
def test_scores_equal_numpy_and_the_point_kernel(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    count = st.count.cpu().numpy()
    usable = np.isin(st.status, (0, 2))
    differing = pairs = 0
    for f, (p, l) in enumerate(SHAPES):
        R, t, d = _seg(st.R, f), _seg(st.t, f), st.scenes[f]
        ip, bp = _point_pred(R, t, st.Kf[f], d)
        il, bl = _line_pred(R, t, st.Kf[f], d)
        ref = (ip.sum(1) + il.sum(1)) * _seg(usable, f)
        slack = (bp.sum(1) + bl.sum(1)) * _seg(usable, f)
        diff = np.abs(_seg(count, f) - ref)
        assert (diff <= slack).all(), (f, np.nonzero(diff > slack)[0][:8])
        differing += int(diff.sum()); pairs += H * (p + l)
    print(f"scores: {differing} differing (hypothesis, correspondence) pairs of {pairs}")
    assert differing <= 1e-6 * pairs, (differing, pairs)
    # scenes without lines: bit for bit what the point-only kernel counts
    only = [f for f, (p, l) in enumerate(SHAPES) if l == 0]
    sc = rn.pack_scenes([st.args[0][f] for f in only], [st.args[2][f] for f in only], st.K[only] if st.per else st.K, device=st.dev)
    sel = torch.cat([torch.arange(f * H, (f + 1) * H) for f in only]).to(st.dev)
    ref = rn.score_scenes(sc, st.res.R[sel].contiguous(), st.res.t[sel].contiguous(), THRESH, status=st.res.status[sel].contiguous(), usable=(0, 2))
    assert torch.equal(ref, st.count[sel])


# ---- 5. selection -------------------------------------------------------------------------------------------------------------------------
def _check_selection(st, count, sel):
    R, t, head, mp, ml = (a.cpu().numpy() for a in sel)
    cnt = count.cpu().numpy()
    diff = 0
    for f in range(F):
        c = _seg(cnt, f)
        hb = int(np.argmax(c))   # (numpy: the first of the maxima)
        assert head[f, 2] == hb and head[f, 3] == int((_seg(st.status, f) == 0).sum()) and head[f, 0] == _seg(st.status, f)[hb], f
        assert np.array_equal(R[f], _seg(st.R, f)[hb], equal_nan=True) and np.array_equal(t[f], _seg(st.t, f)[hb], equal_nan=True), f
        diff += _check_masks(st, f, R[f], t[f], mp, ml, "selection")
        assert head[f, 1] == mp[st.offp[f]:st.offp[f + 1]].sum() + ml[st.offl[f]:st.offl[f + 1]].sum(), f
    return diff


def test_selection_takes_the_first_maximum_and_masks_its_inliers(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    diff = _check_selection(st, st.count, st.sel)
    flat = torch.full_like(st.count, 3)   # all counts equal: the lowest index wins in every scene
    sel = rn.select_pnpl_scenes(st.sc, flat, st.res.R, st.res.t, st.res.status, THRESH)
    assert (sel[2][:, 2] == 0).all()
    diff += _check_selection(st, flat, sel)
    print(f"selection: {diff} mask entries differ from numpy, all borderline")


# ---- 6. consensus assembly ----------------------------------------------------------------------------------------------------------------
def _check_consensus(st, mp, ml, expect_nan=()):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    Bt, Qt, cnt = rn.assemble_pnpl_consensus(st.sc, mp, ml)
    B2, Q2, c2 = rn.assemble_pnpl_consensus(st.sc, mp, ml)
    assert torch.equal(Bt.view(torch.int64), B2.view(torch.int64)) and torch.equal(Qt.view(torch.int64), Q2.view(torch.int64)) and torch.equal(cnt, c2)
    Bn, Qn, mpn, mln = Bt.cpu().numpy(), Qt.cpu().numpy(), mp.cpu().numpy().astype(bool), ml.cpu().numpy().astype(bool)
    nan = []
    for f in range(F):
        d = st.scenes[f]
        kp, kl = mpn[st.offp[f]:st.offp[f + 1]], mln[st.offl[f]:st.offl[f + 1]]
        assert int(cnt[f]) == int(kp.sum() + kl.sum()), f
        if int(cnt[f]) < 3:
            assert np.isnan(Bn[f]).all() and np.isnan(Qn[f]).all(), f
            nan.append(f)
            continue
        Bs, Qs = ca.assemble_batch(d["pts_2d"][kp][None] if kp.any() else None, d["line_2d"][kl][None] if kl.any() else None,
                                   d["pts_3d"][kp][None] if kp.any() else None, d["line_3d"][kl][None] if kl.any() else None, st.Kf[f], device=st.dev,
                                   blocked=False)
        Bs, Qs = Bs.cpu().numpy()[0], Qs.cpu().numpy()[0]
        if not np.isfinite(Qs).all():
            assert np.isnan(Bn[f]).all() and np.isnan(Qn[f]).all(), f
            nan.append(f)
            continue
        assert np.abs(Qn[f] - Qs).max() <= 1e-11 * np.abs(Qs).max(), (f, np.abs(Qn[f] - Qs).max() / np.abs(Qs).max())
        assert np.abs(Bn[f] - Bs).max() <= 1e-9 * max(1.0, np.abs(Bs).max()), (f, np.abs(Bn[f] - Bs).max())
    assert set(expect_nan) <= set(nan), (expect_nan, nan)
    return Bt, Qt, cnt, nan


def test_consensus_assembly_equals_assemble_batch_on_the_masked_sets(st):
    import torch

    _, _, _, nan = _check_consensus(st, st.sel[3], st.sel[4])   # the consensus sets of the selection
    assert all(sum(SHAPES[f]) < 16 for f in nan), nan
    # random subsets, one scene cut down to two correspondences (one point and one line: three RECORDS): NaN for that scene only
    rs = np.random.RandomState(3)
    mp = (rs.rand(int(st.offp[-1])) < 0.5).astype(np.uint8)
    ml = (rs.rand(int(st.offl[-1])) < 0.5).astype(np.uint8)
    j = 10   # (both neighbours are large scenes: half of their correspondences is a well-posed set)
    mp[st.offp[j]:st.offp[j + 1]] = 0; ml[st.offl[j]:st.offl[j + 1]] = 0
    mp[st.offp[j] + 3] = 1; ml[st.offl[j + 1] - 1] = 1
    Bt, Qt, cnt, nan = _check_consensus(st, torch.as_tensor(mp, device=st.dev), torch.as_tensor(ml, device=st.dev), expect_nan=[j])
    assert int(cnt[j]) == 2
    assert torch.isfinite(Qt[j - 1]).all() and torch.isfinite(Qt[j + 1]).all() and torch.isfinite(Bt[j + 1]).all()
    assert all(f == j or sum(SHAPES[f]) < 16 for f in nan), nan


# ---- 7. refit update ----------------------------------------------------------------------------------------------------------------------
def test_refit_update_follows_the_rule(st):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    R, t, head, mp, ml = (a.clone() for a in st.sel)
    Bt, Qt, cnt = rn.assemble_pnpl_consensus(st.sc, mp, ml)
    fit = ca.solve_cost_batch(Qt, Bt)
    cnt = cnt.clone()
    big = [f for f in range(F) if sum(SHAPES[f]) >= 60 and int(fit.status[f]) in (0, 2) and int(cnt[f]) >= 4]
    assert len(big) >= 4, big
    j_status, j_count, j_lose = big[0], big[1], big[2]
    fit.status[j_status] = 3            # an unusable fit
    cnt[j_count] = 3                    # fitted to fewer than four correspondences
    head[j_lose, 1] = sum(SHAPES[j_lose]) + 1   # would lose inliers, whatever it explains
    before = tuple(a.cpu().numpy().copy() for a in (R, t, head, mp, ml))
    rn.refit_update_pnpl_scenes(st.sc, fit, cnt, THRESH, R, t, head, mp, ml)
    after = tuple(a.cpu().numpy() for a in (R, t, head, mp, ml))
    fR, ft, fs, fc = fit.R.cpu().numpy(), fit.t.cpu().numpy(), fit.status.cpu().numpy(), cnt.cpu().numpy()
    taken = 0
    for f in range(F):
        d = st.scenes[f]
        ip, bp = _point_pred(fR[f], ft[f], st.Kf[f], d)
        il, bl = _line_pred(fR[f], ft[f], st.Kf[f], d)
        n_new, slack = int(ip.sum() + il.sum()), int(bp.sum() + bl.sum())
        usable = fs[f] in (0, 2) and fc[f] >= 4
        sp, sl = slice(st.offp[f], st.offp[f + 1]), slice(st.offl[f], st.offl[f + 1])
        changed = not np.array_equal(after[0][f], before[0][f], equal_nan=True)
        if usable and n_new - slack >= before[2][f, 1]:
            assert changed or np.array_equal(fR[f], before[0][f]), f
        if not usable or n_new + slack < before[2][f, 1]:
            assert not changed, f
        if changed:   # pose, status, both masks and count together
            taken += 1
            assert np.array_equal(after[0][f], fR[f]) and np.array_equal(after[1][f], ft[f]) and after[2][f, 0] == fs[f], f
            assert _check_masks(st, f, fR[f], ft[f], after[3], after[4], "refit") <= slack
            assert after[2][f, 1] == after[3][sp].sum() + after[4][sl].sum() and abs(int(after[2][f, 1]) - n_new) <= slack, f
            assert after[2][f, 1] >= before[2][f, 1], f
        else:
            assert all(np.array_equal(after[i][f], before[i][f], equal_nan=True) for i in (0, 1, 2)), f
            assert np.array_equal(after[3][sp], before[3][sp]) and np.array_equal(after[4][sl], before[4][sl]), f
        assert np.array_equal(after[2][f, 2:], before[2][f, 2:]), f
    assert taken >= 1, taken
    for f in (j_status, j_count, j_lose):
        assert np.array_equal(after[0][f], before[0][f]), f


# ---- 8. the whole call --------------------------------------------------------------------------------------------------------------------
KEYS = ("R", "t", "inliers_pts", "inliers_lines", "offsets", "line_offsets", "head")


def _same(a, b):
    import torch

    return all(torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k], b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k])
               for k in KEYS)


def test_whole_call_equals_the_stages_and_itself(st):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    def call(n, **kw):
        a = [x[:n] for x in st.args]
        return rn.ransac_pnpl_batch(*a, st.K[:n] if st.per else st.K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev, **kw)

    out = call(F)
    assert out["R"].shape == (F, 3, 3) and out["t"].shape == (F, 3) and out["inliers_pts"].shape == (st.offp[-1],)
    assert out["inliers_lines"].shape == (st.offl[-1],) and out["offsets"].shape == (F + 1,) and out["line_offsets"].shape == (F + 1,)
    assert all(out[k].shape == (F,) for k in ("n_inliers", "status", "n_certified", "best_index")) and out["head"].shape == (F, 4)
    assert out["sizes"] == tuple(p for p, _ in SHAPES) and out["line_sizes"] == tuple(l for _, l in SHAPES) and out["n_hyp"] == H
    # the stage functions in sequence, bit for bit
    R, t, head, mp, ml = (a.clone() for a in st.sel)
    Bt, Qt, cnt = rn.assemble_pnpl_consensus(st.sc, mp, ml)
    fit = ca.solve_cost_batch(Qt, Bt, eps=1e-9, max_iters=2500)
    rn.refit_update_pnpl_scenes(st.sc, fit, cnt, THRESH, R, t, head, mp, ml)
    assert torch.equal(out["R"].view(torch.int64), R.view(torch.int64)) and torch.equal(out["t"].view(torch.int64), t.view(torch.int64))
    assert torch.equal(out["head"], head.cpu()) and torch.equal(out["inliers_pts"], mp.bool()) and torch.equal(out["inliers_lines"], ml.bool())
    # the invariants of the result
    Rn, tn, mpn, mln = out["R"].cpu().numpy(), out["t"].cpu().numpy(), out["inliers_pts"].cpu().numpy(), out["inliers_lines"].cpu().numpy()
    best = st.count.cpu().numpy().reshape(F, H).max(1)
    for f in range(F):
        _check_masks(st, f, Rn[f], tn[f], mpn, mln, "whole call")
        assert int(out["n_inliers"][f]) == mpn[st.offp[f]:st.offp[f + 1]].sum() + mln[st.offl[f]:st.offl[f + 1]].sum(), f
        assert int(out["n_inliers"][f]) >= best[f], f
    # the packed form gives the same call; two identical calls are bit-identical
    packed = rn.ransac_pnpl_batch(np.concatenate(st.args[0]), np.concatenate(st.args[1]), np.concatenate(st.args[2]), np.concatenate(st.args[3]), st.K,
                                  n_hyp=H, thresh=THRESH, seed=st.seeds, sizes=[p for p, _ in SHAPES], line_sizes=[l for _, l in SHAPES], device=st.dev)
    assert _same(out, packed) and _same(out, call(F))
    # a call on a side stream directly followed by one of a different F gives what each gives alone
    c = call(7)
    side = torch.cuda.Stream(device=st.dev)
    side.wait_stream(torch.cuda.current_stream(st.dev))
    with torch.cuda.stream(side):
        a2 = call(F)
        c2 = call(7)
    side.synchronize()
    assert _same(out, a2) and _same(c, c2)


def test_wrappers_equal_the_batch_call(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    out = rn.ransac_pnpl_batch(*st.args, st.K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev)
    offp, offl = st.offp, st.offl
    for f in (2, 5, 6, 11):   # a mixed minimal scene, lines only, points only, a mixed scene
        p2, l2, p3, l3 = (a[f] for a in st.args)
        one = rn.ransac_pnpl(p2 if len(p2) else None, l2 if len(l2) else None, p3 if len(p3) else None, l3 if len(l3) else None, st.Kf[f], n_hyp=H,
                             thresh=THRESH, seed=st.seeds[f], device=st.dev)
        assert torch.equal(one["R"].view(torch.int64), out["R"][f].view(torch.int64)) and torch.equal(one["t"].view(torch.int64), out["t"][f].view(torch.int64)), f
        assert torch.equal(one["inliers_pts"], out["inliers_pts"][offp[f]:offp[f + 1]]) and torch.equal(one["inliers_lines"], out["inliers_lines"][offl[f]:offl[f + 1]]), f
        assert [one["status"], one["n_inliers"], one["best_index"], one["n_certified"]] == out["head"][f].tolist(), f
    lines_only = [f for f, (p, l) in enumerate(SHAPES) if p == 0]
    assert len(lines_only) >= 3
    l2, l3 = [st.args[1][f] for f in lines_only], [st.args[3][f] for f in lines_only]
    Kl = st.K[lines_only] if st.per else st.K
    a = rn.ransac_pnl_batch(l2, l3, Kl, n_hyp=H, thresh=THRESH, seed=7, device=st.dev)
    b = rn.ransac_pnpl_batch(None, l2, None, l3, Kl, n_hyp=H, thresh=THRESH, seed=7, device=st.dev)
    assert _same(a, b) and a["inliers_pts"].numel() == 0 and a["sizes"] == (0,) * len(lines_only)
    one = rn.ransac_pnl(l2[1], l3[1], Kl[1] if st.per else Kl, n_hyp=H, thresh=THRESH, seed=8, device=st.dev)
    lo = a["line_offsets"].cpu().numpy()
    assert torch.equal(one["inliers_lines"], a["inliers_lines"][lo[1]:lo[2]]) and one["n_inliers"] == int(a["n_inliers"][1])


def test_planted_inliers_are_recovered():
    """Noise-free scenes with at most 30 % clutter, 512 hypotheses: every ground-truth inlier of every scene of at least 20 correspondences
    is in the returned masks.  (512 draws hold no all-inlier set with a chance below (1 - 0.7^4)^512 ~ e^-140: no scene is set aside.)"""
    import torch

    from cvxpnpl_amd import ransac as rn

    scenes, K = _make_scenes(False, seed0=700, sigma=0.0, max_frac=0.3)
    out = rn.ransac_pnpl_batch(*_lists(scenes), K, n_hyp=512, thresh=THRESH, seed=11, device=torch.device("cuda:0"))
    mp, ml = out["inliers_pts"].cpu().numpy(), out["inliers_lines"].cpu().numpy()
    op, ol = out["offsets"].cpu().numpy(), out["line_offsets"].cpu().numpy()
    checked = 0
    for f, d in enumerate(scenes):
        if sum(SHAPES[f]) < 20:
            continue
        checked += 1
        assert (mp[op[f]:op[f + 1]] | ~d["inlier_pts"]).all() and (ml[ol[f]:ol[f + 1]] | ~d["inlier_lines"]).all(), f
        assert int(out["n_inliers"][f]) >= int(d["inlier_pts"].sum() + d["inlier_lines"].sum()), f
    assert checked >= 12, checked


# ---- 9. points only -----------------------------------------------------------------------------------------------------------------------
def test_point_only_scenes_agree_with_ransac_pnp_batch(st):
    from cvxpnpl_amd import ransac as rn, synth

    sizes = [4, 7, 47, 70, 129, 250, 600, 33]
    xs, Xs = [], []
    for i, m in enumerate(sizes):
        d = synth.make_ransac(1, n_corr=m, outlier_frac=0.4 * i / len(sizes) if m > 8 else 0.0, sigma=0.5, seed=900 + i)
        xs.append(d["scene_2d"]); Xs.append(d["scene_3d"])
    K = np.stack([st.Kf[f] for f in range(len(sizes))]) if st.per else st.K
    ref = rn.ransac_pnp_batch(xs, Xs, K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev)
    out = rn.ransac_pnpl_batch(xs, None, Xs, None, K, n_hyp=H, thresh=THRESH, seed=SEED, device=st.dev)
    assert out["inliers_lines"].numel() == 0
    assert np.array_equal(out["best_index"].numpy(), ref["best_index"].numpy()), (out["best_index"], ref["best_index"])
    assert np.array_equal(out["n_inliers"].numpy(), ref["n_inliers"].numpy()), (out["n_inliers"], ref["n_inliers"])
    off = np.concatenate([[0], np.cumsum(sizes)])
    Ra, ta, Rb, tb = out["R"].cpu().numpy(), out["t"].cpu().numpy(), ref["R"].cpu().numpy(), ref["t"].cpu().numpy()
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
    print(f"points only: max geodesic between ransac_pnpl_batch and ransac_pnp_batch {worst:.3e} rad")
    assert worst <= 1e-8, worst
