"""MSAC scoring on the device (ransac_pnp_batch(scoring="msac"), libcvxpnpl_amd_ransac_msac.so).

The scoring stage against the numpy reference (tests/ransac_msac_reference.py) and, for the counts, against the third library's kernel;
the selection and the rounds against the reference's arg-max and replay run on the DEVICE's own gains and counts, which is exact; then
the whole call.  Nine scenes of 4 .. 700 correspondences (exactly 4, around the wave width 64 and around the scoring tile of 512) with
host-made poses around the ground truth, some of them unusable or NaN, one scene wholly behind the camera; once with a shared K and
once with a K per scene."""
import numpy as np
import pytest

from ransac_msac_reference import argmax_first, gain_count_scenes, gain_read, rotation_error_deg, simulate_msac
from test_ransac_msac_library import GAIN_TOL, MARGIN, THRESH, make_case

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 63, 64, 65, 511, 512, 513, 700]
F, H_ALL, BEHIND, CONF = len(SIZES), 300, 1, 0.99   # H_ALL poses per scene: every n_hyp below is a prefix of them; scene BEHIND sees nothing


class _State:
    pass


def _rows(full, n_scenes, act, h0, Hr):
    """rows [f, h0 : h0 + Hr] for f in act of a tensor laid out [n_scenes * H, ...], as one contiguous [len(act) * Hr, ...] tensor"""
    import torch

    H = full.shape[0] // n_scenes
    v = full.reshape((n_scenes, H) + tuple(full.shape[1:]))
    a = torch.as_tensor(np.asarray(act, dtype=np.int64), device=full.device)
    return v[a, h0:h0 + Hr].reshape((len(act) * Hr,) + tuple(full.shape[1:])).contiguous()


@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def st(request):
    """One set of scenes and poses per K mode, computed once with its reference.  Nothing below changes it."""
    import torch

    from cvxpnpl_amd import _lib, ransac as rn

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.ransac_lib(); _lib.ransac_adaptive_lib(); _lib.ransac_msac_lib()
    s = _State()
    s.dev, s.per = torch.device("cuda:0"), request.param == "per_scene_K"
    c = make_case(SIZES, H_ALL, seed=21, per_scene_K=s.per)
    R, t = c["R"].reshape(F, H_ALL, 3, 3).copy(), c["t"].reshape(F, H_ALL, 3).copy()
    R[1::2], t[1::2] = R[1::2, ::-1].copy(), t[1::2, ::-1].copy()   # odd scenes: the good poses come last, so that counts climb over the rounds
    t[BEHIND, :, 2] = -t[BEHIND, :, 2]                               # one scene wholly behind the camera
    status = np.zeros((F, H_ALL), dtype=np.int32)
    status[:, 5::7], status[:, 6::11], status[:, 2::13] = 2, 1, 3   # uncertified (usable), rank > 1 and non-finite (not usable)
    R[:, 9::17] = np.nan                                             # NaN poses under a usable status ...
    status[:, 9::17] = np.where(status[:, 9::17] == 1, 1, 0)
    R[:, 2::13] = np.nan                                             # ... and under status 3
    s.R_h, s.t_h, s.status_h = R.reshape(-1, 3, 3), t.reshape(-1, 3), status
    s.x_h, s.X_h, s.K_h = c["x"], c["X"], c["K"]
    s.ref_gain, s.ref_count, margin = gain_count_scenes(c["x"], c["X"], SIZES, c["K"], s.R_h, s.t_h, THRESH, status=status.reshape(-1))
    assert margin > MARGIN, margin                                   # no residual within rounding of the threshold: equal counts are a fair demand
    s.ref_gain, s.ref_count = s.ref_gain.reshape(F, H_ALL), s.ref_count.reshape(F, H_ALL)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    s.off = off
    s.sc = rn.pack_scenes([c["x"][off[f]:off[f + 1]] for f in range(F)], [c["X"][off[f]:off[f + 1]] for f in range(F)], c["K"], device=s.dev,
                          seeds=list(range(F)))
    s.R = torch.as_tensor(s.R_h, device=s.dev).contiguous()
    s.t = torch.as_tensor(s.t_h, device=s.dev).contiguous()
    s.status = torch.as_tensor(status.reshape(-1), device=s.dev).contiguous()
    s.gain, s.count = rn.score_scenes_msac(s.sc, s.R, s.t, THRESH, status=s.status, usable=(0, 2))
    torch.cuda.synchronize()
    s.gain_h, s.count_h = s.gain.cpu().numpy().reshape(F, H_ALL), s.count.cpu().numpy().reshape(F, H_ALL)
    return s


def _prefix(st, H):
    """the first H poses of every scene: (R, t, status) [F*H, ...]"""
    return tuple(_rows(v, F, range(F), 0, H) for v in (st.R, st.t, st.status))


@pytest.mark.parametrize("H", [1, 255, 256, 257])
def test_scoring_equals_the_reference_and_the_count_kernel(st, H):
    import torch

    from cvxpnpl_amd import ransac as rn

    R, t, status = _prefix(st, H)
    gain, count = rn.score_scenes_msac(st.sc, R, t, THRESH, status=status, usable=(0, 2))
    assert gain.shape == (F * H,) and gain.dtype == torch.float64 and count.shape == (F * H,) and count.dtype == torch.int32
    assert torch.equal(count, rn.score_scenes(st.sc, R, t, THRESH, status=status, usable=(0, 2)))   # the third library's count, exactly
    g, c = gain.cpu().numpy().reshape(F, H), count.cpu().numpy().reshape(F, H)
    worst = float(np.max(np.abs(g - st.ref_gain[:, :H])))
    print(f"H = {H}: worst |gain - reference| {worst:.2e} over gains up to {st.ref_gain[:, :H].max():.1f}")
    assert np.array_equal(c, st.ref_count[:, :H])
    assert worst <= GAIN_TOL, worst
    unusable = np.isin(st.status_h[:, :H], (1, 3))
    assert (g[unusable] == 0.0).all() and (c[unusable] == 0).all() and not np.signbit(g[unusable]).any()
    assert (g[BEHIND] == 0.0).all() and (c[BEHIND] == 0).all()
    assert ((g >= 0) & (g <= c)).all()
    assert np.array_equal(g, st.gain_h[:, :H])           # a pose's gain over a scene does not depend on the launch it is scored in
    # without a status array every live hypothesis is scored: the NaN poses still gain nothing
    g2, c2 = rn.score_scenes_msac(st.sc, R, t, THRESH)
    ref_g, ref_c, _ = gain_count_scenes(st.x_h, st.X_h, SIZES, st.K_h, R.cpu().numpy(), t.cpu().numpy(), THRESH)
    assert np.array_equal(c2.cpu().numpy(), ref_c) and np.max(np.abs(g2.cpu().numpy() - ref_g)) <= GAIN_TOL


def test_active_scoring_is_the_rows_of_the_fixed_scoring_bit_for_bit(st):
    import torch

    from cvxpnpl_amd import ransac as rn

    for act in (list(range(F)), [7, 2, 8, 0, 5, 3, 1, 6, 4], [F - 1], [4, 4, 0]):
        a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
        for h0, Hr in ((0, 1), (0, 64), (3, 257), (44, 256)):
            R, t, s = (_rows(v, F, act, h0, Hr) for v in (st.R, st.t, st.status))
            gain, count = rn.score_active_msac(st.sc, a, len(act), R, t, THRESH, status=s, usable=(0, 2))
            assert torch.equal(gain.view(torch.int64), _rows(st.gain, F, act, h0, Hr).view(torch.int64)), (act, h0, Hr)   # the bits
            assert torch.equal(count, _rows(st.count, F, act, h0, Hr)), (act, h0, Hr)
    # an entry outside [0, F) is skipped: its rows stay as they were
    act = [2, -1, F, 5]
    a = torch.as_tensor(act, dtype=torch.int32, device=st.dev)
    Hr = 70
    R, t, s = (_rows(v, F, [2, 0, 0, 5], 0, Hr) for v in (st.R, st.t, st.status))
    import ctypes as C

    from cvxpnpl_amd import _lib

    L = _lib.ransac_msac_lib()
    gain =torch.full((4 * Hr,), -7.0, dtype=torch.float64, device=st.dev)
    count = torch.full((4 * Hr,), -7, dtype=torch.int32, device=st.dev)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    rc = L.cvxpnpl_ransac_msac_score_active(F, 4, p(a), Hr, p(st.sc.offsets), st.sc.total, p(R), p(t), p(s), 5, p(st.sc.K), st.sc.per_scene_K, p(st.sc.x),
                                            p(st.sc.X), THRESH, p(gain), p(count), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    g, c = gain.reshape(4, Hr), count.reshape(4, Hr)
    assert (g[1:3] == -7.0).all() and (c[1:3] == -7).all()
    assert torch.equal(g[0], st.gain.reshape(F, H_ALL)[2, :Hr]) and torch.equal(g[3], st.gain.reshape(F, H_ALL)[5, :Hr])


def _select_and_check(st, R, t, status, gain, H, want=None):
    """select_scenes_msac on (gain, poses) against the reference's arg-max on the same gains; returns the winners"""
    import torch

    from cvxpnpl_amd import ransac as rn

    oR, ot, head, mask, score = rn.select_scenes_msac(st.sc, gain, R, t, status, THRESH)
    torch.cuda.synchronize()
    g, hd, sc_h, stat = gain.cpu().numpy().reshape(F, H), head.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy().reshape(F, H)
    m = mask.cpu().numpy()
    for f in range(F):
        w = argmax_first(g[f])
        assert hd[f, 2] == w, (f, hd[f], w)
        assert 0 <= hd[f, 2] < H
        assert hd[f, 0] == stat[f, w] and hd[f, 3] == int((stat[f] == 0).sum())
        assert hd[f, 1] == int(m[st.off[f]:st.off[f + 1]].sum())
        assert sc_h[f] == gain_read(g[f])[w] and not np.isnan(sc_h[f])
        assert torch.equal(oR[f], R.reshape(F, H, 3, 3)[f, w]) or bool(torch.isnan(oR[f]).any())
        assert torch.equal(ot[f], t.reshape(F, H, 3)[f, w])
    if want is not None:
        assert list(hd[:, 2]) == list(want), (list(hd[:, 2]), list(want))
    return hd, m, sc_h


@pytest.mark.parametrize("H", [1, 255, 256, 257, 300])
def test_selection_equals_the_reference_argmax_on_the_device_gains(st, H):
    from cvxpnpl_amd import ransac as rn

    R, t, status = _prefix(st, H)
    gain, count = rn.score_scenes_msac(st.sc, R, t, THRESH, status=status, usable=(0, 2))
    hd, m, score = _select_and_check(st, R, t, status, gain, H)
    c = count.cpu().numpy().reshape(F, H)
    for f in range(F):   # a usable winner's mask is the set its count counted
        if st.status_h[f, hd[f, 2]] in (0, 2):
            assert hd[f, 1] == c[f, hd[f, 2]], f
    assert hd[BEHIND, 2] == 0 and hd[BEHIND, 1] == 0 and score[BEHIND] == 0.0   # all gains 0: index 0 wins


def _plant(st, H, slots):
    """every scene's best pose (by the reference) moved to `slots`, its own slot given a poor pose; returns (R, t, status) on the device"""
    import torch

    R, t, s = st.R_h.reshape(F, H_ALL, 3, 3)[:, :H].copy(), st.t_h.reshape(F, H_ALL, 3)[:, :H].copy(), st.status_h[:, :H].copy()
    for f in range(F):
        b = argmax_first(st.ref_gain[f, :H])
        poor = int(np.argmin(np.where(np.isnan(R[f]).any(axis=(1, 2)), np.inf, st.ref_gain[f, :H])))
        Rb, tb = R[f, b].copy(), t[f, b].copy()
        R[f, b], t[f, b], s[f, b] = R[f, poor], t[f, poor], s[f, poor]
        for h in slots:
            R[f, h], t[f, h], s[f, h] = Rb, tb, 0
    return (torch.as_tensor(R.reshape(-1, 3, 3), device=st.dev).contiguous(), torch.as_tensor(t.reshape(-1, 3), device=st.dev).contiguous(),
            torch.as_tensor(s.reshape(-1), device=st.dev).contiguous())


def test_selection_ties_and_the_last_index(st):
    from cvxpnpl_amd import ransac as rn

    H = 300
    # the same pose at h = 3, 67 and 259 -- another lane, another wave, another stride: an exact tie, which the lowest index wins
    R, t, s = _plant(st, H, (3, 67, 259))
    gain, _ = rn.score_scenes_msac(st.sc, R, t, THRESH, status=s, usable=(0, 2))
    g = gain.cpu().numpy().reshape(F, H)
    assert (g[:, 3] == g[:, 67]).all() and (g[:, 3] == g[:, 259]).all()
    hd, _, _ = _select_and_check(st, R, t, s, gain, H)
    seeing = [f for f in range(F) if f != BEHIND]
    assert (hd[seeing, 2] == 3).all(), hd[:, 2]
    assert hd[BEHIND, 2] == 0
    # a unique maximum in the last slot, at every width around the workgroup
    for Hn in (255, 256, 257, 300):
        R, t, s = _plant(st, Hn, (Hn - 1,))
        gain, _ = rn.score_scenes_msac(st.sc, R, t, THRESH, status=s, usable=(0, 2))
        hd, _, _ = _select_and_check(st, R, t, s, gain, Hn)
        assert (hd[seeing, 2] == Hn - 1).all(), (Hn, hd[:, 2])


def test_selection_on_hand_made_gains(st):
    """NaN and negative gains never win, the index stays inside the scene, and all-zero (or all-bad) gains leave index 0."""
    import torch

    H = 300
    R, t, s = _prefix(st, H)
    rs = np.random.RandomState(5)
    g = rs.random_sample((F, H)) * 10
    g[:, ::3] = np.nan
    g[:, 1::3] = -g[:, 1::3] - 1.0
    g[0] = 0.0                                  # all zero
    g[1, :] = np.nan                            # all NaN
    g[2, :] = -np.inf                           # all negative
    g[3, :] = np.nan; g[3, 299] = 1e-300        # one tiny positive gain in the last slot
    g[4, 0] = np.inf                            # an infinite gain is still a gain
    g[5, 17] = g[5, 200] = 11.0                 # a tie across waves and strides
    gain = torch.as_tensor(g.reshape(-1), device=st.dev).contiguous()
    hd, _, score = _select_and_check(st, R, t, s, gain, H)
    assert list(hd[:5, 2]) == [0, 0, 0, 299, 0] and hd[5, 2] == 17
    assert score[0] == 0.0 and score[1] == 0.0 and score[2] == 0.0 and score[3] == 1e-300 and score[4] == np.inf
    for f in range(6, F):
        assert g[f, hd[f, 2]] > 0


def _margins_hold(sim):
    """The condition under which a last-bit difference between the device's and numpy's log cannot flip a decision."""
    for f, drawn, N in sim["margins"]:
        if np.isfinite(N):
            assert abs(drawn - N) > 1e-6 * max(N, 1.0), f"scene {f}: drawn {drawn} against N {N}: change the seed"


def _run_rounds(sc, n_scenes, R, t, status, round_hyp, cap):
    """An MSAC call's rounds over FIXED poses (R, t, status) [n_scenes * H, ...] in place of the sampler and the solver."""
    import torch

    from cvxpnpl_amd import ransac as rn

    def solve(active, A, h0, Hr):
        act = active[:A].cpu().numpy()
        return rn._Fit(*(_rows(v, n_scenes, act, h0, Hr) for v in (R, t, status)))

    state = rn.adaptive_init_msac(sc)
    update = lambda sc_, s_, A, h0, cp, cf, gc, R_, t_, st_, th: rn.update_active_msac(sc_, s_, A, h0, cp, cf, gc[0], gc[1], R_, t_, st_, th)  # noqa: E731
    rounds = rn._rounds(sc, state, (solve, rn.score_active_msac, update), cap, CONF, round_hyp, THRESH)
    torch.cuda.synchronize()
    return state, rounds


@pytest.mark.parametrize("round_hyp", [1, 64])
def test_rounds_hold_what_the_selection_gives_over_the_hypotheses_drawn(st, round_hyp):
    import torch

    from cvxpnpl_amd import ransac as rn

    cap = 256
    sim = simulate_msac(st.gain_h, st.count_h, st.status_h, SIZES, CONF, round_hyp, cap)
    _margins_hold(sim)
    state, rounds = _run_rounds(st.sc, F, st.R, st.t, st.status, round_hyp, cap)
    used, head = state.hyp_used.cpu().numpy(), state.head.cpu().numpy()
    print(f"round_hyp {round_hyp}: hyp_used {list(used)}, winners {list(head[:, 2])}, rounds {rounds}")
    assert rounds == len(sim["active"])
    assert np.array_equal(used, sim["hyp_used"]) and np.array_equal(head[:, 2], sim["winner"]) and np.array_equal(head[:, 3], sim["certified"])
    assert np.array_equal(state.best.cpu().numpy(), sim["best"]) and np.array_equal(state.best_gain.cpu().numpy(), sim["best_gain"])
    assert len(set(used)) >= 3 and (used == cap).any() and (used < cap).any()   # first-round stops, later stops and runs to the cap
    mask = state.mask.cpu().numpy()
    for u in sorted(set(used)):   # a scene that stopped after u hypotheses holds what the selection gives over its first u, bit for bit
        R, t, s = _prefix(st, int(u))
        gain, _ = rn.score_scenes_msac(st.sc, R, t, THRESH, status=s, usable=(0, 2))
        oR, ot, hd, m, score = rn.select_scenes_msac(st.sc, gain, R, t, s, THRESH)
        m = m.cpu().numpy()
        for f in np.nonzero(used == u)[0]:
            assert torch.equal(state.R[f].view(torch.int64), oR[f].view(torch.int64)) and torch.equal(state.t[f], ot[f]), (f, u)
            assert torch.equal(state.head[f, :3], hd[f, :3]) and torch.equal(state.best_gain[f].view(torch.int64), score[f].view(torch.int64)), (f, u)
            assert np.array_equal(mask[st.off[f]:st.off[f + 1]], m[st.off[f]:st.off[f + 1]]), (f, u)


def test_rounds_over_more_scenes_than_one_launch_holds():
    """66 000 scenes of 4 points, 2 hypotheses each: the scoring launches are chunked over scene0 / act0."""
    import torch

    from cvxpnpl_amd import ransac as rn

    n, H, pool = 66000, 2, 16
    c = make_case([4] * pool, H, seed=33, outliers=[0.0, 0.3] * (pool // 2))   # four inliers of four: N = 0, the scene stops after one hypothesis
    rep = n // pool
    x, X = np.tile(c["x"], (rep, 1)), np.tile(c["X"], (rep, 1))
    R, t = np.tile(c["R"], (rep, 1, 1)), np.tile(c["t"], (rep, 1))
    ref_g, ref_c = np.tile(c["gain"].reshape(pool, H), (rep, 1)), np.tile(c["count"].reshape(pool, H), (rep, 1))
    dev = torch.device("cuda:0")
    sc = rn.pack_scenes(x, X, c["K"], sizes=[4] * n, device=dev, seeds=[0] * n)
    Rd, td = torch.as_tensor(R, device=dev).contiguous(), torch.as_tensor(t, device=dev).contiguous()
    status = torch.zeros((n * H,), dtype=torch.int32, device=dev)
    gain, count = rn.score_scenes_msac(sc, Rd, td, THRESH, status=status)
    g, cnt = gain.cpu().numpy().reshape(n, H), count.cpu().numpy().reshape(n, H)
    assert np.array_equal(cnt, ref_c) and np.max(np.abs(g - ref_g)) <= GAIN_TOL
    assert np.array_equal(g[:pool], g[-pool:]) and np.array_equal(g[:pool], g[65536:65536 + pool])   # the second slab computes what the first does
    sim = simulate_msac(g, cnt, np.zeros((n, H), dtype=np.int64), [4] * n, CONF, 1, H)
    state, rounds = _run_rounds(sc, n, Rd, td, status, 1, H)
    used, head = state.hyp_used.cpu().numpy(), state.head.cpu().numpy()
    assert rounds == len(sim["active"]) == 2 and len(sim["active"][1]) not in (0, n)   # some scenes stop after one hypothesis, some go on
    assert np.array_equal(used, sim["hyp_used"]) and np.array_equal(head[:, 2], sim["winner"])
    assert np.array_equal(state.best.cpu().numpy(), sim["best"]) and np.array_equal(state.best_gain.cpu().numpy(), sim["best_gain"])
    oR, ot, hd, m, score = rn.select_scenes_msac(sc, gain, Rd, td, status, THRESH)
    both = torch.as_tensor(used == H, device=dev)
    assert torch.equal(state.R[both], oR[both]) and torch.equal(state.head[both][:, :3], hd[both][:, :3]) and torch.equal(state.best_gain[both], score[both])
    per_scene = state.mask.reshape(n, 4).sum(dim=1).to(torch.int32)
    assert torch.equal(per_scene, state.head[:, 1])


# ---- the whole call

@pytest.fixture(scope="module")
def frames():
    """The 48 scenes of the experiment that motivates the library: 100 correspondences, 30 % clutter, 1 px noise."""
    from cvxpnpl_amd import synth

    ds = [synth.make_ransac(1, n_corr=100, outlier_frac=0.3, sigma=1.0, seed=100 + f) for f in range(48)]
    return [d["scene_2d"] for d in ds], [d["scene_3d"] for d in ds], ds[0]["K"], [d["R_gt"] for d in ds]


def _gain_of(out, xs, Xs, K, thresh):
    """the gain of a call's poses over their scenes, by the scoring kernel"""
    from cvxpnpl_amd import ransac as rn

    sc = rn.pack_scenes(xs, Xs, K, device=out["R"].device)
    return rn.score_scenes_msac(sc, out["R"].contiguous(), out["t"].contiguous(), thresh)[0]


def test_count_scoring_is_the_call_without_the_keyword(frames):
    import torch

    import cvxpnpl_amd as ca

    xs, Xs, K, _ = frames
    for kw in (dict(), dict(confidence=0.99, round_hyp=32), dict(polish=True)):
        a = ca.ransac_pnp_batch(xs[:12], Xs[:12], K, n_hyp=128, thresh=4.0, seed=0, **kw)
        b = ca.ransac_pnp_batch(xs[:12], Xs[:12], K, n_hyp=128, thresh=4.0, seed=0, scoring="count", **kw)
        assert "score" not in b and "scoring" not in b and set(a) == set(b)   # (the keys of a count call are pinned by earlier tests)
        for k in ("R", "t", "inliers", "offsets", "head"):
            assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.bool else a[k], b[k].view(torch.uint8) if b[k].dtype == torch.bool else b[k]), k


@pytest.mark.parametrize("mode", ["fixed", "adaptive", "guided"])
def test_msac_call(frames, mode):
    import torch

    import cvxpnpl_amd as ca

    xs, Xs, K, _ = frames
    n = 16
    rs = np.random.RandomState(3)
    kw = {"fixed": dict(), "adaptive": dict(confidence=0.99, round_hyp=32),
          "guided": dict(quality=[rs.random_sample(100) for _ in range(n)], pool_full=64)}[mode]
    out = ca.ransac_pnp_batch(xs[:n], Xs[:n], K, n_hyp=128, thresh=4.0, seed=0, refit=False, scoring="msac", **kw)
    assert out["scoring"] == "msac" and out["score"].shape == (n,) and out["score"].dtype == torch.float64 and out["score"].is_cuda
    # without a refit the pose is the selected minimal hypothesis: its gain, scored again on its own, is the score bit for bit
    again = _gain_of(out, xs[:n], Xs[:n], K, 4.0)
    assert torch.equal(again.view(torch.int64), out["score"].view(torch.int64))
    assert (out["score"] > 0).all() and (out["score"].cpu() <= out["n_inliers"].double()).all()
    if mode == "adaptive":
        assert (out["hyp_used"] <= 128).all() and (out["hyp_used"] < 128).any() and out["rounds"] >= 1
    else:   # the count call selects among the same draws: its winner cannot gain more
        cnt = ca.ransac_pnp_batch(xs[:n], Xs[:n], K, n_hyp=128, thresh=4.0, seed=0, refit=False, **kw)
        g_cnt = _gain_of(cnt, xs[:n], Xs[:n], K, 4.0)
        assert (out["score"] >= g_cnt).all(), (out["score"] - g_cnt).min()
        assert (cnt["n_inliers"] >= out["n_inliers"]).all()      # ... as the MSAC winner cannot count more
    # refits and polish compose: the score still describes the selected hypothesis
    full = ca.ransac_pnp_batch(xs[:n], Xs[:n], K, n_hyp=128, thresh=4.0, seed=0, refit=True, polish=True, scoring="msac", **kw)
    assert torch.equal(full["score"], out["score"]) and (full["n_inliers"] >= out["n_inliers"]).all()


def test_msac_winner_is_closer_to_the_truth_than_the_count_winner_on_the_device(frames):
    """The experiment of tests/test_ransac_msac_library.py on the device: 48 scenes, 128 hypotheses each, thresh = 4, seed = 0, no refit.
    The MSAC winner's mean rotation error is at most 0.85 of the count winner's."""
    import cvxpnpl_amd as ca

    xs, Xs, K, R_gt = frames
    errs = {}
    for scoring in ("count", "msac"):
        out = ca.ransac_pnp_batch(xs, Xs, K, n_hyp=128, thresh=4.0, seed=0, refit=False, scoring=scoring)
        R = out["R"].cpu().numpy()
        errs[scoring] = np.array([rotation_error_deg(R[f], R_gt[f]) for f in range(48)])
    c, m = errs["count"], errs["msac"]
    print(f"count winner: mean {c.mean():.3f} deg, median {np.median(c):.3f} deg;  MSAC winner: mean {m.mean():.3f} deg, median {np.median(m):.3f} deg;  "
          f"ratio {m.mean() / c.mean():.2f};  MSAC better {int((m < c).sum())}, equal {int((m == c).sum())}, worse {int((m > c).sum())}")
    assert m.mean() <= 0.85 * c.mean(), (m.mean(), c.mean())
