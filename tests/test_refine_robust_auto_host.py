"""The host path of the twelfth library (cvxpnpl_robust_scale_batch_host, cvxpnpl_refine_robust_pp_batch_host,
cvxpnpl_robust_cov_batch_host: the same sources as the device kernels) against the independent references
(tests/refine_robust_auto_reference.py): the scale estimate, its exact median, the loop at a scale per problem against the seventh
library, the sandwich covariance against long-double differences, and a Monte-Carlo check that the covariance is the one the estimates
scatter with.  No GPU needed."""
import numpy as np
import pytest

import refine_robust_auto_cases as ac
import refine_robust_auto_reference as ar
import refine_robust_cases as cs
import refine_reference as ref

SIGMA_RTOL = 1e-9   # the bar tests/test_refine_robust_host.py holds robust_w to
COV_FLOORS = 100.0  # the covariance against the difference reference: this many of the reference's own measured floors (the multiple
                    # tests/test_refine_robust_host.py uses for its gradient)


@pytest.fixture(scope="module")
def ca():
    import cvxpnpl_amd
    from cvxpnpl_amd import build

    build.build_refine_robust()
    build.build_refine_robust_auto()
    return cvxpnpl_amd


def _scale(ca, case, **extra):
    return ca.robust_scale_batch_host(case["R0"], case["t0"], K=case["K"], **ac.pack_kwargs(case), **extra)


def _own_median(sq_row):
    return np.median(sq_row[sq_row >= 0.0])


@pytest.mark.parametrize("case", ac.scale_cases() + [ac.masked()], ids=lambda c: c["name"])
def test_scale_matches_the_reference_and_its_median_is_exact(ca, case):
    got = _scale(ca, case)
    worst = 0.0
    for b in range(len(case["R0"])):
        one = cs.one(case, b)
        sigma, med, s = ar.sigma_hat(case["K"][b], case["R0"][b], case["t0"][b], **one)
        lp, ll, *_ = ar.rr.live_weights(**one)
        live = np.concatenate([lp, ll])
        assert got.status[b] == ar.entry_status(case["K"][b], case["R0"][b], case["t0"][b], **one) == 0
        assert got.n_live[b] == live.sum()
        assert (got.sq[b][~live] == -1.0).all() and (got.sq[b][live] >= 0.0).all()
        np.testing.assert_allclose(got.sq[b][live], s, rtol=1e-9, atol=1e-300)
        worst = max(worst, abs(got.sigma_px[b] - sigma) / sigma)
        assert got.med_sq[b].tobytes() == np.float64(_own_median(got.sq[b])).tobytes()
        assert got.sigma_px[b] == np.sqrt(got.med_sq[b] / ar.CHI2_2_MEDIAN)
    print(f"{case['name']}: worst relative error of sigma {worst:.2e}")
    assert worst <= SIGMA_RTOL


@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("m", (3, 4, 5, 6))
def test_ties(ca, m, split):
    case = ac.ties(m, split)
    got = _scale(ca, case)
    _, med, s = ar.sigma_hat(case["K"][0], case["R0"][0], case["t0"][0], **cs.one(case, 0))
    assert got.status[0] == 0 and got.n_live[0] == m
    assert got.med_sq[0].tobytes() == np.float64(_own_median(got.sq[0])).tobytes()
    assert abs(got.med_sq[0] - med) <= 1e-9 * med
    if not split:
        assert got.med_sq[0] == got.sq[0][0]            # an element of sq, not a mean that rounding moved


def test_statuses_in_the_refinements_order_and_nan_for_what_was_not_estimated(ca):
    base = cs.clean(10, 0, "huber")
    B = 7
    idx = [0] * B
    kw = {"pts_2d": base["kw"]["pts_2d"][idx].copy(), "pts_3d": base["kw"]["pts_3d"][idx].copy()}
    K, R, t = base["K"][idx].copy(), base["R0"][idx].copy(), base["t0"][idx].copy()
    w, mask, status = np.ones((B, 10)), np.ones((B, 10), np.uint8), np.zeros(B, np.int32)
    status[1] = 1                                       # not admitted: admit_mask = 1 admits status 0 only
    R[2, 0, 0] = np.nan                                 # a pose that is not finite
    w[3, 4] = -1.0                                      # a bad weight -- and fewer than 3 live records: the weight speaks first
    mask[3, :8] = 0
    mask[3, 4] = 1
    mask[4, 2:] = 0                                     # two live records
    t[5] = -t[5]                                        # behind the camera
    R[6] = R[6] @ np.diag([1.0, 1.0, -1.0])             # det R < 0
    got = ca.robust_scale_batch_host(R, t, K=K, weights_pts=w, mask_pts=mask, status=status, admit_mask=1, **kw)
    assert got.status.tolist() == [0, 2, 2, 4, 3, 4, 2]
    for b in range(B):
        one = dict(pts_2d=kw["pts_2d"][b], pts_3d=kw["pts_3d"][b], weights_pts=w[b], mask_pts=mask[b])
        if b != 1:
            assert got.status[b] == ar.entry_status(K[b], R[b], t[b], **one), b
        if b == 0:
            assert np.isfinite(got.sigma_px[b]) and (got.sq[b] >= 0).all()
        else:
            assert np.isnan(got.sigma_px[b]) and np.isnan(got.med_sq[b]) and np.isnan(got.sq[b]).all(), b
    assert got.n_live.tolist() == [10, 10, 10, 2, 2, 10, 10]
    alone = ca.robust_scale_batch_host(R[:1], t[:1], K=K[:1], pts_2d=kw["pts_2d"][:1], pts_3d=kw["pts_3d"][:1])
    assert alone.sigma_px[0] == got.sigma_px[0]         # the neighbours are unaffected


@pytest.mark.parametrize("loss", ("l2", "huber", "cauchy"))
def test_uniform_scale_array_is_the_seventh_library_bit_for_bit(ca, loss):
    case = cs.contaminated(loss)
    kw = ac.pack_kwargs(case)
    c = 1.7
    B = len(case["R0"])
    want = ca.refine_pose_batch_robust_host(case["R0"], case["t0"], K=case["K"], loss=loss, scale_px=c, max_iters=cs.MAX_ITERS, **kw)
    for scale in (np.full(B, c), c):
        got = ca.refine_pose_batch_robust_auto_host(case["R0"], case["t0"], K=case["K"], loss=loss, scale_px=scale, max_iters=cs.MAX_ITERS, **kw)
        for name in ("R", "t", "cost", "iters", "status", "n_live", "robust_w", "n_inlier"):
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (name, type(scale))
        assert got.sigma_px is None and got.cov is None
        assert loss == "l2" or (got.scale_px == c).all()                                     # (l2 has no scale: a float is not kept)


@pytest.mark.parametrize("loss", ("huber", "cauchy"))
def test_bad_scale_elements_give_status_4_for_their_problem_only(ca, loss):
    base = cs.clean(10, 0, loss)
    idx = [0, 1, 0, 1, 0]
    kw = {k: v[idx] for k, v in ac.pack_kwargs(base).items()}
    K, R, t = base["K"][idx], base["R0"][idx], base["t0"][idx]
    scale = np.array([1.0, 0.0, -1.0, np.nan, np.inf])
    got = ca.refine_pose_batch_robust_auto_host(R, t, K=K, loss=loss, scale_px=scale, covariance=True, **kw)
    want = ca.refine_pose_batch_robust_host(R[:1], t[:1], K=K[:1], loss=loss, scale_px=1.0, **{k: v[:1] for k, v in kw.items()})
    assert got.status.tolist() == [want.status[0], 4, 4, 4, 4]
    assert got.R[0].tobytes() == want.R[0].tobytes() and got.t[0].tobytes() == want.t[0].tobytes()
    assert got.R[1:].tobytes() == R[1:].tobytes() and got.t[1:].tobytes() == t[1:].tobytes()
    assert np.isnan(got.scale_px[1:]).all() and np.isnan(got.cov[1:]).all() and np.isnan(got.cost[1:]).all() and (got.iters[1:] == 0).all()
    assert np.isnan(got.robust_w[1:]).all() and (got.n_inlier[1:] == 0).all()
    assert got.scale_px[0] == 1.0 and np.isfinite(got.cov[0]).all()
    l2 = ca.refine_pose_batch_robust_auto_host(R, t, K=K, loss="l2", scale_px=scale, **kw)     # l2 does not read the array
    assert (l2.status <= 1).all()


def test_two_rounds_are_two_explicit_calls_and_the_estimate_drives_the_scale(ca):
    case = cs.contaminated("huber")
    kw = ac.pack_kwargs(case)
    got = ca.refine_pose_batch_robust_auto_host(case["R0"], case["t0"], K=case["K"], loss="huber", scale_rounds=2, scale_factor=2.0, scale_floor_px=0.5, **kw)
    R, t, iters = case["R0"], case["t0"], 0
    for _ in range(2):
        est = ca.robust_scale_batch_host(R, t, K=case["K"], **kw)
        scale = np.maximum(2.0 * est.sigma_px, 0.5)
        step = ca.refine_pose_batch_robust_auto_host(R, t, K=case["K"], loss="huber", scale_px=scale, **kw)
        R, t, iters = step.R, step.t, iters + step.iters
    assert got.R.tobytes() == R.tobytes() and got.t.tobytes() == t.tobytes() and (got.iters == iters).all()
    assert got.scale_px.tobytes() == scale.tobytes() and got.sigma_px.tobytes() == est.sigma_px.tobytes()
    assert got.cost.tobytes() == step.cost.tobytes()
    floor = ca.refine_pose_batch_robust_auto_host(case["R0"], case["t0"], K=case["K"], loss="huber", scale_floor_px=1e6, max_iters=1, **kw)
    assert (floor.scale_px == 1e6).all()


@pytest.mark.parametrize("loss", ("l2", "huber", "cauchy"))
@pytest.mark.parametrize("kind,n_p,n_l", ac.COV_CASES)
def test_covariance_matches_the_difference_reference(ca, kind, n_p, n_l, loss):
    case, refs = ac.cov_case(kind, n_p, n_l, loss)
    got = ca.robust_covariance_host(case["R0"], case["t0"], K=case["K"], loss=loss, scale_px=case["delta"], **ac.pack_kwargs(case))
    each = ca.robust_covariance_host(case["R0"], case["t0"], K=case["K"], loss=loss, scale_px=np.full(len(refs), case["delta"]), **ac.pack_kwargs(case))
    assert got.cov.tobytes() == each.cov.tobytes()
    for b, (V, floor, H, Bm) in enumerate(refs):
        assert got.status[b] == 0
        err = np.linalg.norm(got.cov[b] - V) / np.linalg.norm(V)
        print(f"{case['name']} problem {b}: reference floor {floor:.2e}, |cov - V| / |V| {err:.2e} ({err / floor:.1f} floors)")
        assert err <= COV_FLOORS * floor, (err, floor)
        assert np.array_equal(got.cov[b], got.cov[b].T) or np.allclose(got.cov[b], got.cov[b].T, rtol=1e-9, atol=0.0)


@pytest.fixture(scope="module")
def sums_program(tmp_path_factory):
    """tests/hostsim/refine_robust_auto_sums_main.cpp compiled from source: the library's own H and B sums, which the ABI only returns as
    their product"""
    import os
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path_factory.mktemp("sums") / "refine_robust_auto_sums")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "hostsim", "refine_robust_auto_sums_main.cpp")], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]

    def run(K, R, t, loss, delta, pts_2d=None, pts_3d=None, line_2d=None, line_3d=None):
        n_p, n_l = (0 if pts_3d is None else len(pts_3d)), (0 if line_3d is None else len(line_3d))
        nums = [np.asarray(a, float).ravel() for a in (K, R, t, pts_2d, pts_3d, line_2d, line_3d) if a is not None]
        text = f"{ {'l2': 0, 'huber': 1, 'cauchy': 2}[loss]} {delta!r} {n_p} {n_l}\n" + "\n".join(repr(float(x)) for x in np.concatenate(nums))
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr[-500:])
        v = np.array([float(x) for x in p.stdout.split()])
        assert len(v) == 3 + 21 + 21 + 1
        c = v[:3]

        def full(u):
            A = np.zeros((6, 6))
            A[np.triu_indices(6)] = u
            return A + np.triu(A, 1).T

        Rc = np.asarray(R) @ c
        S = np.array([[0.0, -Rc[2], Rc[1]], [Rc[2], 0.0, -Rc[0]], [-Rc[1], Rc[0], 0.0]])
        Mi = np.eye(6)
        Mi[3:, :3] = -S                                   # xi_c = M^-1 xi_pub, M = [[I, 0], [S, I]] (refine_core.h's covariance())
        return Mi.T @ full(v[3:24]) @ Mi, Mi.T @ full(v[24:45]) @ Mi, int(v[45])

    return run


@pytest.mark.parametrize("kind,n_p,n_l", ac.COV_CASES)
def test_under_l2_and_unit_weights_h_and_b_are_each_the_references(sums_program, kind, n_p, n_l):
    """H and B on their own, not only H^-1 B H^-1 (a common factor c in H and c^2 in B would cancel there): the library's 21 + 21 sums,
    brought to the public chart, against the difference reference's H and B, each at 100 of ITS OWN measured floors."""
    case, _ = ac.cov_case(kind, n_p, n_l, "l2")
    assert "weights_pts" not in ac.pack_kwargs(case) and "weights_lines" not in ac.pack_kwargs(case) and "mask_pts" not in ac.pack_kwargs(case)
    for b in range(len(case["R0"])):
        one = cs.one(case, b)
        H_ref, B_ref, floor_h, floor_b = ar.hessian_and_meat(case["K"][b], case["R0"][b], case["t0"][b], "l2", case["delta"], **one)
        H, Bm, n_live = sums_program(case["K"][b], case["R0"][b], case["t0"][b], "l2", case["delta"], **one)
        eh, eb = np.linalg.norm(H - H_ref) / np.linalg.norm(H_ref), np.linalg.norm(Bm - B_ref) / np.linalg.norm(B_ref)
        print(f"{case['name']} problem {b}: H floor {floor_h:.2e} error {eh:.2e} ({eh / floor_h:.1f} floors); B floor {floor_b:.2e} error {eb:.2e} ({eb / floor_b:.1f} floors)")
        assert n_live == n_p + n_l
        assert eh <= COV_FLOORS * floor_h and eb <= COV_FLOORS * floor_b, (eh, floor_h, eb, floor_b)


def test_the_bad_scale_hook_rests_on_the_one_six_wide_sum_of_the_loop():
    """PerProblemScale raises the sixth of robust_problem's centre sums, which it knows as the only sum<6> of the loop.  A second six-wide
    sum in refine_robust_core.h, or centre sums of another width, would corrupt or drop status 4 silently: this pins the dependency (the
    drop is also what test_bad_scale_elements_give_status_4_for_their_problem_only would show)."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "cvxpnpl_amd", "csrc", "refine_robust_core.h")).read()
    body = src[src.index("CVX_HD void robust_problem("):src.index("CVX_HD int robust_weights_problem(")]
    widths = re.findall(r"sum<([^>]+)>", body)
    assert widths.count("6") == 1 and "s6[5] > 0.0" in body, widths
    assert set(widths) == {"6", "1", "ACC_N - 1"}, widths                                   # the loop's other sums: 1 and 27 wide


def test_covariance_statuses(ca):
    case, _ = ac.cov_case("clean", 10, 0, "huber")
    kw = ac.pack_kwargs(case)
    idx = [0] * 6
    K, R, t = case["K"][idx].copy(), case["R0"][idx].copy(), case["t0"][idx].copy()
    p2, p3 = kw["pts_2d"][idx].copy(), kw["pts_3d"][idx].copy()
    status = np.array([0, 1, 3, 0, 0, 0], np.int32)
    mask, w = np.ones((6, 10), np.uint8), np.ones((6, 10))
    mask[3, 3:] = 0                                     # three live records: m = 6
    w[4, 0] = np.inf                                    # a bad weight
    R[5], t[5] = cs.clean(10, 0, "huber")["R0"][0], cs.clean(10, 0, "huber")["t0"][0]
    got = ca.robust_covariance_host(R, t, pts_2d=p2, pts_3d=p3, K=K, loss="huber", scale_px=case["delta"], status=status, mask_pts=mask, weights_pts=w)
    assert got.status[:5].tolist() == [0, 0, 2, 3, 4]
    assert got.cov[0].tobytes() == got.cov[1].tobytes() and np.isfinite(got.cov[0]).all()
    assert np.isnan(got.cov[2:5]).all()
    assert got.status[5] in (0, 3) and (got.status[5] == 0) == bool(np.isfinite(got.cov[5]).all())   # a pose off the minimum: H decides
    bad = ca.robust_covariance_host(R[:2], t[:2], pts_2d=p2[:2], pts_3d=p3[:2], K=K[:2], loss="huber", scale_px=np.array([case["delta"], 0.0]))
    assert bad.status.tolist() == [0, 4] and np.isnan(bad.cov[1]).all() and bad.cov[0].tobytes() == got.cov[0].tobytes()


MC_DRAWS, MC_N, MC_SIGMA = 2000, 100, 2.0


def _mc_scene(contaminated):
    rs = np.random.RandomState(2024)
    K = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])
    R = ref.expm_so3(np.array([0.3, -0.2, 0.1]))
    t = np.array([0.1, -0.2, 6.0])
    X = rs.uniform(-2.0, 2.0, (MC_N, 3))
    h = (X @ R.T + t) @ K.T
    x0 = h[:, :2] / h[:, 2:]
    x = x0[None] + rs.normal(0.0, MC_SIGMA, (MC_DRAWS, MC_N, 2))
    if contaminated:                                    # 20 % of the points displaced by up to 100 px in a direction of their own, anew in every draw
        n_out = MC_N // 5
        ang, mag = rs.uniform(0.0, 2.0 * np.pi, (MC_DRAWS, n_out)), rs.uniform(0.0, 100.0, (MC_DRAWS, n_out))
        x[:, :n_out] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    return K, R, t, X, x


def _log_so3(Q):
    w = np.stack([Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]], -1) * 0.5
    s = np.linalg.norm(w, axis=1)
    th = np.arcsin(np.clip(s, 0.0, 1.0))
    return w * np.where(s > 1e-12, th / np.maximum(s, 1e-300), 1.0)[:, None]


@pytest.mark.parametrize("contaminated", (False, True), ids=("clean", "contaminated"))
@pytest.mark.parametrize("loss", ("huber", "cauchy"))
def test_monte_carlo_the_estimates_scatter_with_the_returned_covariance(ca, loss, contaminated):
    """100 points at sigma = 2 px, 2000 noise draws of one scene, the scale from the estimate: every diagonal entry of the empirical
    covariance of (log(R_hat R^T), t_hat - t) over the mean returned covariance lies in [0.8, 1.25] (sampling error of a variance ratio
    at 2000 draws: 3.2 %; H^-1 alone would give about 0.25)."""
    K, R, t, X, x = _mc_scene(contaminated)
    B = MC_DRAWS
    got = ca.refine_pose_batch_robust_auto_host(np.tile(R, (B, 1, 1)), np.tile(t, (B, 1)), pts_2d=x, pts_3d=np.tile(X, (B, 1, 1)), K=K, loss=loss,
                                                covariance=True, max_iters=50)
    assert (got.status <= 1).all() and np.isfinite(got.cov).all()
    xi = np.concatenate([_log_so3(got.R @ R.T), got.t - t], 1)
    emp = np.var(xi, axis=0, ddof=1)
    ratio = emp / np.diagonal(got.cov, axis1=1, axis2=2).mean(0)
    print(f"{loss} {'contaminated' if contaminated else 'clean'}: sigma_hat {got.sigma_px.mean():.3f}, variance ratios {np.round(ratio, 3)}")
    assert (ratio >= 0.8).all() and (ratio <= 1.25).all(), ratio
