"""Local optimisation in adaptive RANSAC over points and lines on the device (ransac_pnpl_batch(confidence=..., local_opt=...),
libcvxpnpl_amd_ransac_pnpl_lo.so).

The assembly of a step against the fourth library's consensus assembly on the numpy reference's masks
(tests/ransac_pnpl_lo_reference.py), and on a points-only scene set against the fourteenth library's assembly; the update on planted
fits against the reference's rule; the rounds against the reference's replay run on the DEVICE's own counts, which is exact; then the
whole call against the theorem: the draws do not depend on LO and the running best with LO is never below the plain one, so no scene
draws more, and a scene that stops after u hypotheses holds at least the inliers of the fixed budget u.  Twelve scenes: the nine (P, L) of
the library test (every branch of the centre rule, the 64-lane and the 256-lane boundary), one of which one point and one line are taken,
one behind the camera at its running pose and one with a degenerate 2D line; once with a shared K and once with a K per scene."""
import numpy as np
import pytest

from ransac_adaptive_reference import needed
from ransac_lo_reference import take_fit
from ransac_pnpl_lo_reference import simulate_lo
from test_ransac_pnpl_lo_library import CLUTTER, MARGIN, SHAPES as LIB_SHAPES, THRESH, WIDEN, assert_cost_close, make_case, reference_masks

pytestmark = pytest.mark.gpu

SHAPES = list(LIB_SHAPES) + [(70, 60), (40, 30), (200, 100)]
F, TWO, BEHIND, DEG, CONF = len(SHAPES), 9, 10, 11, 0.99
M = [p + l for p, l in SHAPES]


def build_case(per_scene_K):
    """The scenes and their running poses (host arrays; needs no GPU): make_case, then scene TWO keeps one point and one line of those
    its running pose takes and has the others moved 500 px off, the running pose of scene BEHIND looks away from its scene, and one line
    that the running pose of scene DEG takes gets a = b."""
    c = make_case(SHAPES, seed=9, per_scene_K=per_scene_K, outliers=CLUTTER + (0.3,) * 3)
    op, ol = c["off_p"], c["off_l"]
    mp, ml = c["masks"][THRESH]
    sp, sl = slice(op[TWO], op[TWO + 1]), slice(ol[TWO], ol[TWO + 1])
    c["x"][sp][np.setdiff1d(np.arange(SHAPES[TWO][0]), np.flatnonzero(mp[sp])[:1])] += 500.0
    c["l2"][sl][np.setdiff1d(np.arange(SHAPES[TWO][1]), np.flatnonzero(ml[sl])[:1])] += np.array([[500.0, 0.0], [0.0, 500.0]])
    c["t"][BEHIND] = -c["t"][BEHIND]
    sd = slice(ol[DEG], ol[DEG + 1])
    c["deg"] = int(np.flatnonzero(ml[sd])[0])
    c["l2"][sd][c["deg"], 1] = c["l2"][sd][c["deg"], 0]
    margin = np.inf
    for th in list(c["masks"]):
        p, l, m = reference_masks(c, c["R"], c["t"], th)
        c["masks"][th], margin = (p, l), min(margin, m)
    gp, gl, m = reference_masks(c, c["R_gt"], c["t_gt"], THRESH)   # the planted fits of the update test are the true poses
    c["gt_masks"] = (gp, gl)
    assert min(margin, m) > MARGIN, (margin, m)
    return c


def scene_count(c, masks, f):
    return int(masks[0][c["off_p"][f]:c["off_p"][f + 1]].sum()) + int(masks[1][c["off_l"][f]:c["off_l"][f + 1]].sum())


def planted_update(c):
    """The update test's plan (host arrays; needs no GPU): the active list, per entry the planted fit (R, t, status, cnt), and per scene
    the planted state (best = head[:, 1], hyp_used) with done flags per entry; then what the reference's rule makes of it."""
    n_run = np.array([scene_count(c, c["masks"][THRESH], f) for f in range(F)])
    n_gt = np.array([scene_count(c, c["gt_masks"], f) for f in range(F)])
    active = np.array([6, 5, 8, 7, F + 5, DEG, BEHIND, 3, -1], dtype=np.int32)   # (two entries outside [0, F))
    A = len(active)
    inside = [0 <= f < F for f in active]
    fit_R = np.stack([c["R_gt"][f] if ok else np.eye(3) for f, ok in zip(active, inside)])
    fit_t = np.stack([c["t_gt"][f] if ok else np.zeros(3) for f, ok in zip(active, inside)])
    fit_status, fit_cnt = np.zeros(A, dtype=np.int32), np.full(A, 50, dtype=np.int32)
    best = n_run.copy()
    best[5] = n_gt[5]            # an equal count: taken, the tie goes to the fit (status 2: usable)
    fit_status[1] = 2
    best[8] = n_gt[8] + 1        # one inlier short: not taken
    fit_status[3] = 3            # status 3: not taken
    fit_cnt[5] = 3               # fitted to three: not taken
    best[BEHIND] = 0             # the scene behind the camera counted nothing so far
    fit_R[7] = np.nan            # a NaN pose under a usable status: counts nothing, not taken
    best[3] = max(best[3], 1)
    assert n_gt[6] >= n_run[6] and n_gt[BEHIND] > 0 and n_gt[DEG] >= n_run[DEG]
    take = np.array([ok and take_fit(fit_status[a], fit_cnt[a], 0 if np.isnan(fit_R[a]).any() else n_gt[f], best[f])
                     for a, (f, ok) in enumerate(zip(active, inside))])
    assert list(take) == [True, True, False, False, False, False, True, False, False]
    best_after = best.copy()
    for a, f in enumerate(active):
        if take[a]:
            best_after[f] = n_gt[f]
    # hyp_used: scene 6 exactly where the rule starts to hold at its NEW best (and not at the old one), scene 5 one draw before it
    # holds, scene 8 far below (its flag is already set and stays), the others far below
    hyp_used = np.full(F, 1, dtype=np.int32)
    N6, N5 = needed(best_after[6], M[6], CONF), needed(best_after[5], M[5], CONF)
    hyp_used[6], hyp_used[5] = int(np.ceil(N6)), int(np.ceil(N5)) - 1
    assert hyp_used[6] >= N6 and (best[6] == best_after[6] or hyp_used[6] < needed(best[6], M[6], CONF)) and 0 < hyp_used[5] < N5
    done0 = np.zeros(A, dtype=np.int32)
    done0[2] = 1
    return dict(active=active, fit_R=fit_R, fit_t=fit_t, fit_status=fit_status, fit_cnt=fit_cnt, best=best, best_after=best_after, take=take,
                hyp_used=hyp_used, done0=done0, n_gt=n_gt, cap=1000)


class _State:
    pass


def _pack(c, dev, seeds=None):
    from cvxpnpl_amd import ransac as rn

    op, ol = c["off_p"], c["off_l"]
    n = len(c["shapes"])
    return rn.pack_pnpl_scenes([c["x"][op[f]:op[f + 1]] for f in range(n)], [c["l2"][ol[f]:ol[f + 1]] for f in range(n)],
                               [c["X"][op[f]:op[f + 1]] for f in range(n)], [c["l3"][ol[f]:ol[f + 1]] for f in range(n)], c["K"], device=dev,
                               seeds=list(range(n)) if seeds is None else seeds)


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One set of scenes and running poses per K mode, on the device once, with the reference's masks.  Nothing below changes it."""
    import torch

    from cvxpnpl_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_pnpl_lib(); _lib.ransac_adaptive_lib(); _lib.ransac_pnpl_adaptive_lib(); _lib.ransac_lo_lib(); _lib.ransac_pnpl_lo_lib()
    s = _State()
    s.dev, s.per = torch.device("cuda:0"), request.param == "per_scene_K"
    s.c = c = build_case(s.per)
    s.sc = _pack(c, s.dev)
    s.R, s.t = torch.as_tensor(c["R"], device=s.dev).contiguous(), torch.as_tensor(c["t"], device=s.dev).contiguous()
    torch.cuda.synchronize()
    return s


def _state(st, active, best=None, head=None, mask=None, mask_lines=None, hyp_used=None, done=None):
    """a fresh state over st's scenes with the running poses and the given active list (at most F entries, padded to F) planted"""
    import torch

    from cvxpnpl_amd import ransac as rn

    s = rn.lo_init(st.sc, rn.adaptive_pnpl_init(st.sc))
    s.R.copy_(st.R); s.t.copy_(st.t)
    act = np.zeros(F, dtype=np.int32)
    act[:len(active)] = active
    s.active = torch.as_tensor(act, device=st.dev)
    for name, v in (("best", best), ("head", head), ("mask", mask), ("mask_lines", mask_lines), ("hyp_used", hyp_used), ("done", done)):
        if v is not None:
            getattr(s, name).copy_(torch.as_tensor(v, device=st.dev))
    return s


@pytest.mark.parametrize("m_k", WIDEN)
def test_assembly_equals_the_consensus_assembly_of_the_reference_set(st, m_k):
    import torch

    from cvxpnpl_amd import ransac as rn

    th, c = THRESH * m_k, st.c
    mp_h, ml_h = c["masks"][th]
    mp, ml = torch.as_tensor(mp_h.astype(np.uint8), device=st.dev), torch.as_tensor(ml_h.astype(np.uint8), device=st.dev)
    Bc, Qc, cc = rn.assemble_pnpl_consensus(st.sc, mp, ml)      # the fourth library on the reference's masks: [F, ...]
    assert np.array_equal(cc.cpu().numpy(), [scene_count(c, (mp_h, ml_h), f) for f in range(F)])
    seen = set()
    for active in ([6, F, 0, 5, 8, 7, 1, 11], [2, 4, -1, 3, 10, 9]):   # both shorter than F, each with an entry outside [0, F)
        A = len(active)
        s = _state(st, active)
        out = (torch.full((A, 27), 7.0, dtype=torch.float64, device=st.dev), torch.full((A, 45), 7.0, dtype=torch.float64, device=st.dev),
               torch.full((A,), -7, dtype=torch.int32, device=st.dev))
        Bt, Qt, cnt = rn.lo_assemble_pnpl_active(st.sc, s, A, th, out=out)
        again = rn.lo_assemble_pnpl_active(st.sc, s, A, th)
        torch.cuda.synchronize()
        for a, f in enumerate(active):
            if not 0 <= f < F:                                  # skipped, not clamped: its rows stay untouched bit for bit
                assert (Bt[a] == 7.0).all() and (Qt[a] == 7.0).all() and int(cnt[a]) == -7, a
                continue
            seen.add(f)
            assert int(cnt[a]) == int(cc[f]), (f, int(cnt[a]), int(cc[f]))          # exact
            assert torch.equal(Bt[a], again[0][a]) or torch.isnan(Bt[a]).all()      # the same bits from launch to launch
            assert torch.equal(Qt[a], again[1][a]) or torch.isnan(Qt[a]).all()
            if torch.isnan(Qc[f]).any():
                assert torch.isnan(Bt[a]).all() and torch.isnan(Qt[a]).all(), f
            else:
                assert_cost_close(Bt[a].cpu().numpy(), Qt[a].cpu().numpy(), Bc[f].cpu().numpy(), Qc[f].cpu().numpy(), (f, m_k))
    assert seen == set(range(F))
    assert int(cc[BEHIND]) == 0 and int(cc[TWO]) == 2 and torch.isnan(Qc[TWO]).all() and torch.isnan(Qc[BEHIND]).all()
    assert not ml_h[c["off_l"][DEG] + c["deg"]]                                      # the degenerate line is never taken
    assert sum(not torch.isnan(Qc[f]).any() for f in range(F)) >= F - 3             # (a scene of four may take fewer than three)
    # the host entry computes the same
    Bh, Qh, ch = rn.lo_assemble_pnpl_host(c["x"], c["X"], c["l2"], c["l3"], c["sizes"], c["line_sizes"], c["K"], c["R"], c["t"], np.arange(F), th)
    for f in range(F):
        assert int(ch[f]) == int(cc[f]), f
        if torch.isnan(Qc[f]).any():
            assert np.isnan(Bh[f]).all() and np.isnan(Qh[f]).all(), f
        else:
            assert_cost_close(Bh[f], Qh[f], Bc[f].cpu().numpy(), Qc[f].cpu().numpy(), ("host", f, m_k))


def test_points_only_assembly_equals_the_point_librarys():
    """A scene set without lines through both assemblies: the same counts, the costs within the assembly tolerance.  Whether the bits
    are equal is printed, not required: the two kernels are compiled apart."""
    import torch

    from cvxpnpl_amd import ransac as rn
    from test_ransac_lo_library import make_case as make_point_case

    dev = torch.device("cuda:0")
    sizes = (4, 63, 65, 513, 700)
    c = make_point_case(sizes, seed=21, thresholds=(THRESH, 2 * THRESH))
    off = c["off"]
    xs, Xs = [c["x"][off[f]:off[f + 1]] for f in range(len(sizes))], [c["X"][off[f]:off[f + 1]] for f in range(len(sizes))]
    sp = rn.pack_scenes(xs, Xs, c["K"], device=dev, seeds=list(range(len(sizes))))
    sl = rn.pack_pnpl_scenes(xs, None, Xs, None, c["K"], device=dev, seeds=list(range(len(sizes))))
    a, b = rn.lo_init(sp, rn.adaptive_init(sp)), rn.lo_init(sl, rn.adaptive_pnpl_init(sl))
    for s in (a, b):
        s.R.copy_(torch.as_tensor(c["R"], device=dev)); s.t.copy_(torch.as_tensor(c["t"], device=dev))
    for th in (THRESH, 2 * THRESH):
        Bp, Qp, cp = rn.lo_assemble_active(sp, a, len(sizes), th)
        Bl, Ql, cl = rn.lo_assemble_pnpl_active(sl, b, len(sizes), th)
        torch.cuda.synchronize()
        assert torch.equal(cp, cl) and int((cp >= 3).sum()) >= len(sizes) - 1
        same = True
        for f in range(len(sizes)):
            if torch.isnan(Qp[f]).any():
                assert torch.isnan(Ql[f]).all() and torch.isnan(Bl[f]).all(), f
                continue
            assert_cost_close(Bl[f].cpu().numpy(), Ql[f].cpu().numpy(), Bp[f].cpu().numpy(), Qp[f].cpu().numpy(), (f, th))
            same = same and torch.equal(Bl[f], Bp[f]) and torch.equal(Ql[f], Qp[f])
        print(f"points-only set at thresh {th}: bits equal to lo_assemble_active: {same}")


def test_update_takes_a_planted_fit_exactly_where_the_rule_says(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    c, op, ol = st.c, st.c["off_p"], st.c["off_l"]
    p = planted_update(c)
    active, A = p["active"], len(p["active"])
    head = np.zeros((F, 4), dtype=np.int32)
    head[:, 1], head[:, 2], head[:, 3] = p["best"], 5, 7
    s = _state(st, active, best=p["best"].astype(np.int32), head=head, mask=c["masks"][THRESH][0].astype(np.uint8),
               mask_lines=c["masks"][THRESH][1].astype(np.uint8), hyp_used=p["hyp_used"], done=np.concatenate([p["done0"], np.zeros(F - A, dtype=np.int32)]))
    before = {k: getattr(s, k).clone() for k in ("R", "t", "head", "best", "mask", "mask_lines", "lo_taken", "done", "hyp_used")}

    class fit:
        R, t = torch.as_tensor(p["fit_R"], device=st.dev).contiguous(), torch.as_tensor(p["fit_t"], device=st.dev).contiguous()
        status = torch.as_tensor(p["fit_status"], device=st.dev)

    cnt = torch.as_tensor(p["fit_cnt"], device=st.dev)
    rn.lo_update_pnpl_active(st.sc, s, A, p["cap"], CONF, fit, cnt, THRESH)
    torch.cuda.synchronize()
    gp, gl = (torch.as_tensor(m.astype(np.uint8), device=st.dev) for m in c["gt_masks"])
    bits = lambda v: v.contiguous().view(torch.int64)  # noqa: E731
    for a, f in enumerate(active):
        if not 0 <= f < F:
            assert int(s.done[a]) == int(before["done"][a]), a
            continue
        sp, sl = slice(op[f], op[f + 1]), slice(ol[f], ol[f + 1])
        if p["take"][a]:
            assert torch.equal(s.R[f], fit.R[a]) and torch.equal(s.t[f], fit.t[a]), f
            assert s.head[f].tolist() == [int(p["fit_status"][a]), int(p["n_gt"][f]), 5, 7], (f, s.head[f].tolist())
            assert int(s.best[f]) == int(p["n_gt"][f]) and int(s.lo_taken[f]) == 1, f
            assert torch.equal(s.mask[sp], gp[sp]) and torch.equal(s.mask_lines[sl], gl[sl]), f      # both masks equal the reference's
        else:   # unchanged bit for bit
            assert torch.equal(bits(s.R[f]), bits(before["R"][f])) and torch.equal(bits(s.t[f]), bits(before["t"][f])), f
            assert torch.equal(s.head[f], before["head"][f]) and int(s.best[f]) == int(before["best"][f]) and int(s.lo_taken[f]) == 0, f
            assert torch.equal(s.mask[sp], before["mask"][sp]) and torch.equal(s.mask_lines[sl], before["mask_lines"][sl]), f
        N = needed(p["best_after"][f], M[f], CONF)
        assert abs(rn.needed_hypotheses(int(p["best_after"][f]), M[f], CONF) - N) <= 1e-9 * max(N, 1.0) or N == np.inf
        want = int(bool(p["done0"][a]) or p["hyp_used"][f] >= p["cap"] or p["hyp_used"][f] >= N)
        assert int(s.done[a]) == want, (a, f, int(s.done[a]), want, N)
    untouched = sorted(set(range(F)) - set(int(f) for f in active))
    assert TWO in untouched
    for f in untouched:   # a scene that is not in the list: unchanged
        sp, sl = slice(op[f], op[f + 1]), slice(ol[f], ol[f + 1])
        assert torch.equal(bits(s.R[f]), bits(before["R"][f])) and torch.equal(s.head[f], before["head"][f]) and int(s.lo_taken[f]) == 0, f
        assert torch.equal(s.mask[sp], before["mask"][sp]) and torch.equal(s.mask_lines[sl], before["mask_lines"][sl]) and int(s.best[f]) == int(before["best"][f])
    assert torch.equal(s.hyp_used, before["hyp_used"]) and torch.equal(s.done[A:], before["done"][A:])
    done = s.done.cpu().numpy()[:A]
    assert done[0] == 1 and p["done0"][0] == 0      # flipped 0 -> 1 exactly at ceil(N) of the new best over P_f + L_f
    assert done[1] == 0                              # one draw before the rule holds
    assert done[2] == 1 and p["done0"][2] == 1      # a flag that is set stays set
    # a state that did not go through lo_init, or without a line mask, is refused
    s.lo_taken = None
    with pytest.raises(ValueError, match="lo_taken"):
        rn.lo_update_pnpl_active(st.sc, s, A, p["cap"], CONF, fit, cnt, THRESH)
    s.mask_lines = None
    with pytest.raises(TypeError, match="mask_lines"):
        rn.lo_assemble_pnpl_active(st.sc, s, A, THRESH)


# ---- the rounds and the whole call: frames of 40 points + 20 lines

def _frames(n, outlier_frac, seed0=100, n_pts=40, n_lines=20):
    from cvxpnpl_amd import synth

    fr = outlier_frac if isinstance(outlier_frac, (list, tuple)) else [outlier_frac] * n
    ds = [synth.make_ransac_pnpl(n_pts=n_pts, n_lines=n_lines, outlier_frac=fr[f], sigma=1.0, seed=seed0 + f) for f in range(n)]
    return [d["pts_2d"] for d in ds], [d["line_2d"] for d in ds], [d["pts_3d"] for d in ds], [d["line_3d"] for d in ds]


@pytest.mark.parametrize("round_hyp", [1, 64])
def test_rounds_equal_the_replay_on_the_devices_own_counts(round_hyp):
    """The loop of ransac_pnpl_batch(confidence=..., local_opt=2, lo_widen=1.5) by the stage wrappers, every count it acts on read back:
    the reference's replay on those counts, with M_f = P_f + L_f, must arrive at the same state after the same rounds."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn, synth

    dev, cap, n_lo, Fr = torch.device("cuda:0"), 256, 2, 6
    sc = rn.pack_pnpl_scenes(*_frames(Fr, [0.2, 0.4, 0.5, 0.6, 0.7, 0.5]), synth.K_KINECT, device=dev, seeds=list(range(Fr)))
    state = rn.lo_init(sc, rn.adaptive_pnpl_init(sc))
    steps = rn.lo_thresholds(THRESH, n_lo, 1.5)
    max_rounds = -(-cap // round_hyp)
    counts, status = np.zeros((Fr, cap), dtype=np.int64), np.full((Fr, cap), 3, dtype=np.int64)
    lo_counts, lo_usable = np.zeros((Fr, max_rounds, n_lo), dtype=np.int64), np.zeros((Fr, max_rounds, n_lo), dtype=bool)
    actives, A, h0, r = [], Fr, 0, 0
    while A > 0 and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        act = state.active[:A].cpu().numpy().copy()
        actives.append(act)
        res = rn.solve_minimal_costs(*rn.sample_assemble_active(sc, state.active, A, h0, Hr, cap), eps=1e-6, max_iters=100, device=dev)
        count = rn.score_pnpl_active(sc, state.active, A, res.R, res.t, THRESH, status=res.status, usable=(0, 2))
        counts[act, h0:h0 + Hr] = count.cpu().numpy().reshape(A, Hr)
        status[act, h0:h0 + Hr] = res.status.cpu().numpy().reshape(A, Hr)
        rn.update_pnpl_active(sc, state, A, h0, cap, CONF, count, res.R, res.t, res.status, THRESH)
        for k, th_k in enumerate(steps):
            Bt, Qt, cnt = rn.lo_assemble_pnpl_active(sc, state, A, th_k)
            fit = ca.solve_cost_batch(Qt, Bt, eps=1e-6, max_iters=100, device=dev)
            lo_counts[act, r, k] = rn.score_pnpl_active(sc, state.active, A, fit.R, fit.t, THRESH).cpu().numpy()   # the count kernel on the refits
            lo_usable[act, r, k] = (np.isin(fit.status.cpu().numpy(), (0, 2))) & (cnt.cpu().numpy() >= 4)
            rn.lo_update_pnpl_active(sc, state, A, cap, CONF, fit, cnt, THRESH)
        rn.compact_active(sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
        h0, r = h0 + Hr, r + 1
    ref = simulate_lo(counts, status, [60] * Fr, lo_counts, lo_usable, CONF, round_hyp, cap)
    assert r == len(ref["active"]) and all(np.array_equal(a, b) for a, b in zip(actives, ref["active"])), (r, len(ref["active"]))
    head = state.head.cpu().numpy()
    assert np.array_equal(state.hyp_used.cpu().numpy(), ref["hyp_used"]) and np.array_equal(state.best.cpu().numpy(), ref["best"])
    assert np.array_equal(head[:, 1], ref["best"]) and np.array_equal(head[:, 2], ref["winner"]) and np.array_equal(head[:, 3], ref["certified"])
    assert np.array_equal(state.lo_taken.cpu().numpy(), ref["lo_taken"])
    n_mask = state.mask.view(Fr, 40).sum(dim=1).cpu().numpy() + state.mask_lines.view(Fr, 20).sum(dim=1).cpu().numpy()
    assert np.array_equal(n_mask, ref["best"])                                       # both masks and the count agree
    print(f"rounds of {round_hyp}: {r} rounds, hyp_used {ref['hyp_used'].tolist()}, best {ref['best'].tolist()}, refits taken {ref['lo_taken'].tolist()}")
    assert ref["lo_taken"].sum() > 0 and len(set(ref["hyp_used"].tolist())) > 1


N_FRAMES, CAP = 16, 1024


@pytest.fixture(scope="module")
def calls():
    """16 frames of 40 points + 20 lines with mixed clutter (0 ... 60 %), the plain adaptive call and the LO calls, once."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = _State()
    s.frames = _frames(N_FRAMES, [0.6 * f / (N_FRAMES - 1) for f in range(N_FRAMES)])
    s.kw = dict(n_hyp=CAP, thresh=THRESH, seed=0, refit=False, confidence=CONF, round_hyp=64, device=torch.device("cuda:0"))
    s.call = lambda **kw: rn.ransac_pnpl_batch(*s.frames, synth.K_KINECT, **{**s.kw, **kw})  # noqa: E731
    s.plain = s.call()
    s.lo = {1: s.call(local_opt=1, lo_widen=2.0), 3: s.call(local_opt=3, lo_widen=2.0)}
    s.fixed = {}
    return s


def _same(a, b):
    """two results: the same keys, every tensor the same bits (a NaN equals the same NaN)"""
    import torch

    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
            bits = (lambda v: v.contiguous().view(torch.int64)) if a[k].dtype == torch.float64 else (lambda v: v)
            assert torch.equal(bits(a[k]), bits(b[k])), k
        else:
            assert a[k] == b[k], k


def test_local_opt_0_is_todays_call_key_for_key(calls):
    out = calls.call(local_opt=0, lo_widen=3.0)
    _same(out, calls.plain)
    assert "lo_taken" not in out and "local_opt" not in out and "lo_widen" not in out
    _same(calls.call(local_opt=0, refit=True, polish=True), calls.call(refit=True, polish=True))
    _same(calls.call(local_opt=0, confidence=None, n_hyp=64), calls.call(confidence=None, n_hyp=64))


@pytest.mark.parametrize("n", [1, 3])
def test_no_scene_draws_more_and_none_holds_less_than_its_fixed_budget(calls, n):
    import torch

    lo, plain = calls.lo[n], calls.plain
    assert lo["local_opt"] == n and lo["lo_widen"] == 2.0 and lo["lo_taken"].dtype == torch.int32 and lo["lo_taken"].shape == (N_FRAMES,)
    assert set(lo) == set(plain) | {"lo_taken", "local_opt", "lo_widen"}
    used_l, used_p = lo["hyp_used"].numpy(), plain["hyp_used"].numpy()
    print(f"local_opt={n}: hypotheses {used_p.sum()} -> {used_l.sum()} (ratio {used_l.sum() / used_p.sum():.3f}), rounds {plain['rounds']} -> {lo['rounds']}, "
          f"mean inliers {plain['n_inliers'].double().mean():.1f} -> {lo['n_inliers'].double().mean():.1f}, refits taken {int(lo['lo_taken'].sum())}")
    assert (used_l <= used_p).all(), (used_l, used_p)
    for u in sorted(set(used_l.tolist())):   # the fixed budget u, for the scenes that stopped there
        if u not in calls.fixed:
            calls.fixed[u] = calls.call(n_hyp=int(u), confidence=None)["n_inliers"].numpy()
        at = used_l == u
        assert (lo["n_inliers"].numpy()[at] >= calls.fixed[u][at]).all(), (u, lo["n_inliers"].numpy()[at], calls.fixed[u][at])
    assert int(lo["lo_taken"].sum()) > 0
    n_mask = lo["inliers_pts"].view(torch.uint8).view(N_FRAMES, 40).sum(dim=1).cpu().numpy() + lo["inliers_lines"].view(torch.uint8).view(N_FRAMES, 20).sum(dim=1).cpu().numpy()
    assert (lo["n_inliers"].numpy() == n_mask).all()   # both masks and the count agree


def test_identical_calls_give_identical_bits_quality_composes_and_lines_alone_run(calls):
    from cvxpnpl_amd import ransac as rn, synth

    _same(calls.call(local_opt=3, lo_widen=2.0), calls.lo[3])
    rs = np.random.RandomState(4)
    quality, line_quality = [rs.random_sample(40) for _ in range(N_FRAMES)], [rs.random_sample(20) for _ in range(N_FRAMES)]
    plain = calls.call(quality=quality, line_quality=line_quality, pool_full=256)
    lo = calls.call(quality=quality, line_quality=line_quality, pool_full=256, local_opt=3, lo_widen=2.0)
    assert lo["pool_full"] == plain["pool_full"] == 256 and (lo["hyp_used"].numpy() <= plain["hyp_used"].numpy()).all()
    assert set(lo) == set(plain) | {"lo_taken", "local_opt", "lo_widen"} and int(lo["lo_taken"].sum()) > 0
    # a lines-only set through ransac_pnl_batch, and one scene through ransac_pnpl
    _, l2, _, l3 = _frames(4, 0.3, seed0=300, n_pts=0, n_lines=40)
    kw = {k: v for k, v in calls.kw.items() if k != "refit"}
    out = rn.ransac_pnl_batch(l2, l3, synth.K_KINECT, local_opt=1, **kw)
    base = rn.ransac_pnl_batch(l2, l3, synth.K_KINECT, **kw)
    assert out["local_opt"] == 1 and out["lo_taken"].shape == (4,) and (out["hyp_used"].numpy() <= base["hyp_used"].numpy()).all()
    assert (out["n_inliers"].numpy() >= 20).all() and out["inliers_pts"].numel() == 0
    one = rn.ransac_pnpl(calls.frames[0][9], calls.frames[1][9], calls.frames[2][9], calls.frames[3][9], synth.K_KINECT, local_opt=3, lo_widen=2.0, **calls.kw)
    assert isinstance(one["lo_taken"], int) and one["local_opt"] == 3 and one["lo_widen"] == 2.0 and 0 < one["hyp_used"] <= CAP
