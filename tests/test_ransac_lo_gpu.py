"""Local optimisation in adaptive RANSAC on the device (ransac_pnp_batch(confidence=..., local_opt=...), libcvxpnpl_amd_ransac_lo.so;
DESIGN.md section 24).

The assembly of a step against the third library's consensus assembly on the numpy reference's mask (tests/ransac_lo_reference.py) and
the host entry against cvxpnpl_amd.api.assemble_subsets on the same mask; the update on planted fits against the reference's rule; the
rounds against the reference's replay run on the DEVICE's own counts, which is exact; then the whole call against the theorem: the draws
do not depend on LO and the running best with LO is never below the plain one, so no scene draws more, and a scene that stops after u
hypotheses holds at least the inliers of the fixed budget u.  Nine scenes of 4 .. 700 correspondences (exactly 4, around the wave width
64, around two passes of the 256-lane workgroup, 700), one behind the camera at its running pose and one of which only two
correspondences are taken; once with a shared K and once with a K per scene."""
import numpy as np
import pytest

from ransac_adaptive_reference import needed
from ransac_lo_reference import simulate_lo, take_fit, taken
from test_ransac_lo_library import MARGIN, SIZES as LIB_SIZES, THRESH, WIDEN, assert_cost_close, make_case, reference_masks, scene_K

pytestmark = pytest.mark.gpu

SIZES = list(LIB_SIZES) + [130, 65]
F, TWO, BEHIND, CONF = len(SIZES), 7, 8, 0.99   # scene TWO: two correspondences taken; scene BEHIND: behind the camera at its running pose


def build_case(per_scene_K):
    """The scenes and their running poses (host arrays; needs no GPU): make_case, then scene TWO keeps two of the correspondences its
    running pose takes and has the others moved 500 px off, and the running pose of scene BEHIND looks away from its scene."""
    c = make_case(SIZES, seed=9, per_scene_K=per_scene_K)
    off = c["off"]
    s = slice(off[TWO], off[TWO + 1])
    keep = np.flatnonzero(c["masks"][THRESH][s])[:2]
    c["x"][s][np.setdiff1d(np.arange(SIZES[TWO]), keep)] += 500.0
    c["t"][BEHIND] = -c["t"][BEHIND]
    margin = np.inf
    for th in list(c["masks"]):
        c["masks"][th], m = reference_masks(c, c["R"], c["t"], th)
        margin = min(margin, m)
    c["gt_mask"], m = reference_masks(c, c["R_gt"], c["t_gt"], THRESH)   # the planted fits of the update test are the true poses
    assert min(margin, m) > MARGIN, (margin, m)
    return c


def planted_update(c):
    """The update test's plan (host arrays; needs no GPU): the active list, per entry the planted fit (R, t, status, cnt), and per scene
    the planted state (best = head[:, 1], hyp_used) with done flags per entry; then what the reference's rule makes of it."""
    off = c["off"]
    n_run = np.array([int(c["masks"][THRESH][off[f]:off[f + 1]].sum()) for f in range(F)])
    n_gt = np.array([int(c["gt_mask"][off[f]:off[f + 1]].sum()) for f in range(F)])
    active = np.array([6, 5, 4, 3, 2, 1, F + 5, 0, 8], dtype=np.int32)   # (F entries: one outside [0, F), scene TWO left out)
    A = len(active)
    fit_R, fit_t = np.stack([c["R_gt"][f] if 0 <= f < F else np.eye(3) for f in active]), np.stack([c["t_gt"][f] if 0 <= f < F else np.zeros(3) for f in active])
    fit_status, fit_cnt = np.zeros(A, dtype=np.int32), np.full(A, 50, dtype=np.int32)
    best = n_run.copy()
    best[5] = n_gt[5]            # an equal count: taken, the tie goes to the fit (status 2: usable)
    fit_status[1] = 2
    best[4] = n_gt[4] + 1        # one inlier short: not taken
    fit_status[3] = 3            # status 3: not taken
    fit_cnt[4] = 3               # fitted to three: not taken
    fit_R[5] = np.nan            # a NaN pose under a usable status: counts nothing, not taken
    fit_cnt[7] = 4               # the scene of four, fitted to four
    best[8] = 0                  # the scene behind the camera counted nothing so far
    assert n_gt[6] >= n_run[6] and n_gt[8] > 0 and n_run[1] > 0
    take = np.array([0 <= f < F and take_fit(fit_status[a], fit_cnt[a], 0 if np.isnan(fit_R[a]).any() else n_gt[f], best[f]) for a, f in enumerate(active)])
    assert list(take) == [True, True, False, False, False, False, False, bool(n_gt[0] >= n_run[0]), True]
    best_after = best.copy()
    for a, f in enumerate(active):
        if take[a]:
            best_after[f] = n_gt[f]
    # hyp_used: scene 6 exactly where the rule starts to hold at its NEW best (and not at the old one), scene 5 one draw before it
    # holds, scene 4 far below (its flag is already set and stays), the others far below
    hyp_used = np.full(F, 1, dtype=np.int32)
    N6, N5 = needed(best_after[6], SIZES[6], CONF), needed(best_after[5], SIZES[5], CONF)
    hyp_used[6], hyp_used[5] = int(np.ceil(N6)), int(np.ceil(N5)) - 1
    assert hyp_used[6] >= N6 and (best[6] == best_after[6] or hyp_used[6] < needed(best[6], SIZES[6], CONF)) and 0 < hyp_used[5] < N5
    done0 = np.zeros(A, dtype=np.int32)
    done0[2] = 1
    return dict(active=active, fit_R=fit_R, fit_t=fit_t, fit_status=fit_status, fit_cnt=fit_cnt, best=best, best_after=best_after, take=take,
                hyp_used=hyp_used, done0=done0, n_gt=n_gt, cap=1000)


class _State:
    pass


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One set of scenes and running poses per K mode, on the device once, with the reference's masks.  Nothing below changes it."""
    import torch

    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib(); _lib.ransac_lib(); _lib.ransac_adaptive_lib(); _lib.ransac_lo_lib()
    s = _State()
    s.dev, s.per = torch.device("cuda:0"), request.param == "per_scene_K"
    s.c = c = build_case(s.per)
    s.off = off = c["off"]
    s.sc = rn.pack_scenes([c["x"][off[f]:off[f + 1]] for f in range(F)], [c["X"][off[f]:off[f + 1]] for f in range(F)], c["K"], device=s.dev,
                          seeds=list(range(F)))
    s.R, s.t = torch.as_tensor(c["R"], device=s.dev).contiguous(), torch.as_tensor(c["t"], device=s.dev).contiguous()
    torch.cuda.synchronize()
    return s


def _state(st, active, best=None, head=None, mask=None, hyp_used=None, done=None):
    """a fresh state over st's scenes with the running poses and the given active list (at most F entries, padded to F) planted"""
    import torch

    from cvxpnpl_amd import ransac as rn

    s = rn.lo_init(st.sc, rn.adaptive_init(st.sc))
    s.R.copy_(st.R); s.t.copy_(st.t)
    act = np.zeros(F, dtype=np.int32)
    act[:len(active)] = active
    s.active = torch.as_tensor(act, device=st.dev)
    for name, v in (("best", best), ("head", head), ("mask", mask), ("hyp_used", hyp_used), ("done", done)):
        if v is not None:
            getattr(s, name).copy_(torch.as_tensor(v, device=st.dev))
    return s


@pytest.mark.parametrize("m_k", WIDEN)
def test_assembly_equals_the_consensus_assembly_of_the_reference_set(st, m_k):
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn

    th, c, off = THRESH * m_k, st.c, st.off
    mask_h = c["masks"][th]
    mask = torch.as_tensor(mask_h.astype(np.uint8), device=st.dev)
    Bc, Qc, cc = rn.assemble_consensus(st.sc, mask)            # the third library on the reference's mask: [F, ...]
    assert np.array_equal(cc.cpu().numpy(), [int(mask_h[off[f]:off[f + 1]].sum()) for f in range(F)])
    seen = set()
    for active in ([6, 99, 0, 5, 8, 7, 1], [2, 4, -1, 3]):     # both shorter than F, each with an entry outside [0, F)
        A = len(active)
        s = _state(st, active)
        out = (torch.full((A, 27), 7.0, dtype=torch.float64, device=st.dev), torch.full((A, 45), 7.0, dtype=torch.float64, device=st.dev),
               torch.full((A,), -7, dtype=torch.int32, device=st.dev))
        Bt, Qt, cnt = rn.lo_assemble_active(st.sc, s, A, th, out=out)
        again = rn.lo_assemble_active(st.sc, s, A, th)
        torch.cuda.synchronize()
        for a, f in enumerate(active):
            if not 0 <= f < F:                                  # skipped, not clamped: its rows stay untouched
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
    # the host entry against cvxpnpl_amd.api.assemble_subsets on the same mask
    Bh, Qh, ch = rn.lo_assemble_host(c["x"], c["X"], SIZES, c["K"], c["R"], c["t"], np.arange(F), th)
    for f in range(F):
        sl = slice(off[f], off[f + 1])
        Bs, Qs, cs = ca.assemble_subsets(torch.as_tensor(c["x"][sl], device=st.dev), torch.as_tensor(c["X"][sl], device=st.dev),
                                         torch.as_tensor(scene_K(c, f), device=st.dev), mask[sl][None])
        assert int(ch[f]) == int(cs[0]), f
        if torch.isnan(Qs).any():
            assert np.isnan(Bh[f]).all() and np.isnan(Qh[f]).all(), f
        else:
            assert_cost_close(Bh[f], Qh[f], Bs[0].cpu().numpy(), Qs[0].cpu().numpy(), ("host", f, m_k))


def test_update_takes_a_planted_fit_exactly_where_the_rule_says(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    c, off = st.c, st.off
    p = planted_update(c)
    active, A = p["active"], len(p["active"])
    head = np.zeros((F, 4), dtype=np.int32)
    head[:, 1], head[:, 2], head[:, 3] = p["best"], 5, 7
    assert A == F
    s = _state(st, active, best=p["best"].astype(np.int32), head=head, mask=c["masks"][THRESH].astype(np.uint8), hyp_used=p["hyp_used"], done=p["done0"])
    before = {k: getattr(s, k).clone() for k in ("R", "t", "head", "best", "mask", "lo_taken", "done", "hyp_used")}

    class fit:
        R, t = torch.as_tensor(p["fit_R"], device=st.dev).contiguous(), torch.as_tensor(p["fit_t"], device=st.dev).contiguous()
        status = torch.as_tensor(p["fit_status"], device=st.dev)

    cnt = torch.as_tensor(p["fit_cnt"], device=st.dev)
    rn.lo_update_active(st.sc, s, A, p["cap"], CONF, fit, cnt, THRESH)
    torch.cuda.synchronize()
    gt_mask = torch.as_tensor(c["gt_mask"].astype(np.uint8), device=st.dev)
    for a, f in enumerate(active):
        if not 0 <= f < F:
            assert int(s.done[a]) == int(before["done"][a]), a
            continue
        sl = slice(off[f], off[f + 1])
        if p["take"][a]:
            assert torch.equal(s.R[f], fit.R[a]) and torch.equal(s.t[f], fit.t[a]), f
            assert s.head[f].tolist() == [int(p["fit_status"][a]), int(p["n_gt"][f]), 5, 7], (f, s.head[f].tolist())
            assert int(s.best[f]) == int(p["n_gt"][f]) and int(s.lo_taken[f]) == 1, f
            assert torch.equal(s.mask[sl], gt_mask[sl]), f
        else:   # unchanged bit for bit
            assert torch.equal(s.R[f].view(torch.int64), before["R"][f].view(torch.int64)) and torch.equal(s.t[f], before["t"][f]), f
            assert torch.equal(s.head[f], before["head"][f]) and int(s.best[f]) == int(before["best"][f]) and int(s.lo_taken[f]) == 0, f
            assert torch.equal(s.mask[sl], before["mask"][sl]), f
        N = rn.needed_hypotheses(int(p["best_after"][f]), SIZES[f], CONF)
        assert N == needed(p["best_after"][f], SIZES[f], CONF) or abs(N - needed(p["best_after"][f], SIZES[f], CONF)) <= 1e-9 * N
        want = int(bool(p["done0"][a]) or p["hyp_used"][f] >= p["cap"] or p["hyp_used"][f] >= N)
        assert int(s.done[a]) == want, (a, f, int(s.done[a]), want, N)
    sl = slice(off[TWO], off[TWO + 1])   # a scene that is not in the list: unchanged
    assert TWO not in active and torch.equal(s.R[TWO], before["R"][TWO]) and torch.equal(s.head[TWO], before["head"][TWO])
    assert torch.equal(s.mask[sl], before["mask"][sl]) and int(s.best[TWO]) == int(before["best"][TWO]) and int(s.lo_taken[TWO]) == 0
    assert torch.equal(s.hyp_used, before["hyp_used"])
    done = s.done.cpu().numpy()[:A]
    assert done[0] == 1 and p["done0"][0] == 0      # flipped 0 -> 1 exactly at ceil(N) of the new best
    assert done[1] == 0                              # one draw before the rule holds
    assert done[2] == 1 and p["done0"][2] == 1      # a flag that is set stays set
    # a state that did not go through lo_init is refused
    s.lo_taken = None
    with pytest.raises(ValueError, match="lo_taken"):
        rn.lo_update_active(st.sc, s, A, p["cap"], CONF, fit, cnt, THRESH)


# ---- the rounds and the whole call: frames of 100 correspondences

def _frames(n, outlier_frac, per_scene_K=False, seed0=100):
    from cvxpnpl_amd import synth

    fr = outlier_frac if isinstance(outlier_frac, (list, tuple)) else [outlier_frac] * n
    ds = [synth.make_ransac(1, n_corr=100, outlier_frac=fr[f], sigma=1.0, seed=seed0 + f) for f in range(n)]
    return [d["scene_2d"] for d in ds], [d["scene_3d"] for d in ds]


@pytest.mark.parametrize("round_hyp", [1, 64])
def test_rounds_equal_the_replay_on_the_devices_own_counts(round_hyp):
    """The loop of ransac_pnp_batch(confidence=..., local_opt=2, lo_widen=1.5) by the stage wrappers, every count it acts on read back:
    the reference's replay on those counts must arrive at the same state after the same rounds."""
    import torch

    import cvxpnpl_amd as ca
    from cvxpnpl_amd import ransac as rn, synth

    dev, cap, n_lo, Fr = torch.device("cuda:0"), 256, 2, 6
    xs, Xs = _frames(Fr, [0.2, 0.4, 0.5, 0.6, 0.7, 0.5])
    sc = rn.pack_scenes(xs, Xs, synth.K_KINECT, device=dev, seeds=list(range(Fr)))
    state = rn.lo_init(sc, rn.adaptive_init(sc))
    steps = rn.lo_thresholds(THRESH, n_lo, 1.5)
    max_rounds = -(-cap // round_hyp)
    counts, status = np.zeros((Fr, cap), dtype=np.int64), np.full((Fr, cap), 3, dtype=np.int64)
    lo_counts, lo_usable = np.zeros((Fr, max_rounds, n_lo), dtype=np.int64), np.zeros((Fr, max_rounds, n_lo), dtype=bool)
    actives, A, h0, r = [], Fr, 0, 0
    while A > 0 and h0 < cap:
        Hr = min(round_hyp, cap - h0)
        act = state.active[:A].cpu().numpy().copy()
        actives.append(act)
        res = ca.pnp_batch(*rn.sample_active(sc, state.active, A, h0, Hr, cap)[:2], sc.K, eps=1e-6, max_iters=100, device=dev)
        count = rn.score_active(sc, state.active, A, res.R, res.t, THRESH, status=res.status, usable=(0, 2))
        counts[act, h0:h0 + Hr] = count.cpu().numpy().reshape(A, Hr)
        status[act, h0:h0 + Hr] = res.status.cpu().numpy().reshape(A, Hr)
        rn.update_active(sc, state, A, h0, cap, CONF, count, res.R, res.t, res.status, THRESH)
        for k, th_k in enumerate(steps):
            Bt, Qt, cnt = rn.lo_assemble_active(sc, state, A, th_k)
            fit = ca.solve_cost_batch(Qt, Bt, eps=1e-6, max_iters=100, device=dev)
            lo_counts[act, r, k] = rn.score_active(sc, state.active, A, fit.R, fit.t, THRESH).cpu().numpy()   # the count kernel on the refits
            lo_usable[act, r, k] = (np.isin(fit.status.cpu().numpy(), (0, 2))) & (cnt.cpu().numpy() >= 4)
            rn.lo_update_active(sc, state, A, cap, CONF, fit, cnt, THRESH)
        rn.compact_active(sc, state, A)
        A = int(state.n_active.cpu()[0])
        state.swap()
        h0, r = h0 + Hr, r + 1
    ref = simulate_lo(counts, status, [100] * Fr, lo_counts, lo_usable, CONF, round_hyp, cap)
    assert r == len(ref["active"]) and all(np.array_equal(a, b) for a, b in zip(actives, ref["active"])), (r, len(ref["active"]))
    head = state.head.cpu().numpy()
    assert np.array_equal(state.hyp_used.cpu().numpy(), ref["hyp_used"]) and np.array_equal(state.best.cpu().numpy(), ref["best"])
    assert np.array_equal(head[:, 1], ref["best"]) and np.array_equal(head[:, 2], ref["winner"]) and np.array_equal(head[:, 3], ref["certified"])
    assert np.array_equal(state.lo_taken.cpu().numpy(), ref["lo_taken"])
    print(f"rounds of {round_hyp}: {r} rounds, hyp_used {ref['hyp_used'].tolist()}, best {ref['best'].tolist()}, refits taken {ref['lo_taken'].tolist()}")
    assert ref["lo_taken"].sum() > 0 and len(set(ref["hyp_used"].tolist())) > 1


N_FRAMES, CAP = 24, 1024


@pytest.fixture(scope="module")
def calls():
    """The 50 % set of the experiment (24 frames of 100 correspondences), the plain adaptive call and the LO calls, once."""
    import torch

    from cvxpnpl_amd import ransac as rn, synth

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = _State()
    s.xs, s.Xs = _frames(N_FRAMES, 0.5)
    s.kw = dict(n_hyp=CAP, thresh=THRESH, seed=0, refit=False, confidence=CONF, round_hyp=64, device=torch.device("cuda:0"))
    s.call = lambda **kw: rn.ransac_pnp_batch(s.xs, s.Xs, synth.K_KINECT, **{**s.kw, **kw})  # noqa: E731
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
    assert int((lo["lo_taken"] > 0).sum()) >= 1
    assert (lo["n_inliers"].numpy() == lo["inliers"].view(torch.uint8).cpu().numpy().reshape(N_FRAMES, 100).sum(axis=1)).all()   # mask and count agree
    assert used_l.sum() < used_p.sum()


def test_identical_calls_give_identical_bits_and_quality_composes(calls):
    _same(calls.call(local_opt=3, lo_widen=2.0), calls.lo[3])
    rs = np.random.RandomState(4)
    quality = [rs.random_sample(100) for _ in range(N_FRAMES)]
    plain = calls.call(quality=quality, pool_full=256)
    lo = calls.call(quality=quality, pool_full=256, local_opt=3, lo_widen=2.0)
    assert lo["pool_full"] == plain["pool_full"] == 256 and (lo["hyp_used"].numpy() <= plain["hyp_used"].numpy()).all()
    assert set(lo) == set(plain) | {"lo_taken", "local_opt", "lo_widen"} and int(lo["lo_taken"].sum()) > 0
