"""cvxpnpl_refine_robust_batch_host (the source of the robust refinement kernels, on host threads) against the independent numpy reference
(tests/refine_robust_reference.py) on the cases of tests/refine_robust_cases.py, its reductions to the least-squares library, and the
properties of the weights.  No GPU needed.

Bars.  Statuses and n_live: equal.  The reference's next robust step from a returned pose: 1e-6 (the project's parity bar, measured as
tests/test_refine_host.py does).  Costs: 1e-9 relative -- except the cost AFTER of the minimal shapes (3 points, 3 lines: six residuals, six
unknowns), whose minimum is an exact fit: two runs that stop at different distances from a cost of zero agree in no digit of it, so there
both costs are held below 1e-9 of the cost before.  robust_w: 1e-9; n_inlier: exact where no s_k is within 1e-6 of delta^2 (asserted per
case; elsewhere by at most the records that are).  The difference gradient of the cost (of rho itself, never rho') relative to
sum |J| |r| omega: 100 x the largest value the reference's own minima give on the same cases, measured in the same way.

Measured: worst next step 1.3e-7; gradient ratio 8.8e-7 at the host's poses against 8.7e-7 at the reference's own minima (bar 8.7e-5;
the two agree to two digits problem by problem); costs within 3.6e-13; robust_w within 6.0e-14; every case converges, the slowest
(Cauchy, 6 lines, delta = 1 px) in 78 trials -- without the rho'' term the iteration is linear near a minimum with records on the curved
part of the loss."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as rc
import refine_robust_cases as cases
import refine_robust_reference as rr

CASES = cases.all_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def rb():
    from cvxpnpl_amd import build, refine_robust

    build.build_refine()              # (the least-squares library: what loss="l2" is held against)
    build.build_refine_robust()
    return refine_robust


def run_host(rb, case, **extra):
    kw = dict(max_iters=cases.MAX_ITERS)
    kw.update(extra)
    return rb.refine_pose_batch_robust_host(case["R0"], case["t0"], K=case["K"], loss=case["loss"], scale_px=case["delta"], **kw, **case["kw"])


@pytest.fixture(scope="module")
def runs(rb):
    """Every case refined once on the host, shared by the tests below."""
    return {c["name"]: run_host(rb, c) for c in CASES}


def grad_h(case):
    """The step of the cost's differences.  l2: 1e-3, as the residuals' Jacobian.  cauchy: rho is analytic in s / delta^2 only within
    |s| < delta^2, i.e. within delta / |J| ~ 1 px / 500 px per rad = 2e-3 rad of the pose, and the stencil spans 3 h: 1e-5 (truncation
    (3 h / 2e-3)^6 ~ 1e-11 of the gradient's terms, rounding eps_long / h ~ 1e-14).  huber: rho'' jumps at delta, a record whose kink lies
    inside the stencil spoils any difference formula, and the chance of that is proportional to h: 1e-8 (rounding 1e-11 of the terms)."""
    return {"l2": 1e-3, "cauchy": 1e-5, "huber": 1e-8}[case["loss"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_status_counts_costs_and_weights_equal_the_references(runs, case):
    out, refs = runs[case["name"]], cases.reference_runs(case)
    for b, r in enumerate(refs):
        assert out.status[b] == r["status"] == 0 and out.n_live[b] == r["n_live"], (b, out.status[b], r["status"])
        assert abs(out.cost[b, 0] - r["cost"][0]) <= 1e-9 * r["cost"][0]
        if case["minimal"]:
            assert out.cost[b, 1] <= 1e-9 * r["cost"][0] and r["cost"][1] <= 1e-9 * r["cost"][0], (out.cost[b], r["cost"])
        else:
            assert abs(out.cost[b, 1] - r["cost"][1]) <= 1e-9 * r["cost"][1], (out.cost[b], r["cost"])
        assert out.cost[b, 1] <= out.cost[b, 0]
        # rho' and the inlier count of the reference AT THE RETURNED POSE
        w, n_in, s = rr.robust_w_full(case["K"][b], out.R[b], out.t[b], case["loss"], case["delta"], **cases.one(case, b))
        assert np.abs(out.robust_w[b] - w).max() <= 1e-9, np.abs(out.robust_w[b] - w).max()
        near = 0 if case["loss"] == "l2" else int((np.abs(s - case["delta"] ** 2) <= 1e-6).sum())
        assert abs(int(out.n_inlier[b]) - n_in) <= near, (out.n_inlier[b], n_in, near)
        if case["loss"] == "l2":
            assert out.n_inlier[b] == out.n_live[b]


def test_n_inlier_is_exact_on_the_cases_built_away_from_delta(runs):
    """The contaminated cases: no s_k within 1e-6 of delta^2 at the returned pose (asserted), so the count is exact."""
    for loss in ("huber", "cauchy"):
        case = cases.contaminated(loss)
        out = runs[case["name"]]
        for b in range(len(out.R)):
            _, n_in, s = rr.robust_w_full(case["K"][b], out.R[b], out.t[b], loss, case["delta"], **cases.one(case, b))
            assert (np.abs(s - case["delta"] ** 2) > 1e-6).all()
            assert out.n_inlier[b] == n_in


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_next_step_from_the_returned_pose(runs, case):
    out = runs[case["name"]]
    worst = max(float(np.linalg.norm(rr.lm_step(case["K"][b], out.R[b], out.t[b], case["loss"], case["delta"], **cases.one(case, b))[0]))
                for b in range(len(out.R)))
    print(f"{case['name']}: iters <= {out.iters.max()}, reference's next step <= {worst:.2e}")
    assert worst <= rc.STEP_BAR
    assert np.abs(np.swapaxes(out.R, 1, 2) @ out.R - np.eye(3)).max() <= 1e-13


def _grad_ratio(case, b, R, t):
    g, scale = rr.cost_gradient(case["K"][b], R, t, case["loss"], case["delta"], h=grad_h(case), **cases.one(case, b))
    return float(np.linalg.norm(g) / scale)


def test_difference_gradient_of_the_cost_vanishes_at_the_returned_pose(runs):
    """d cost / d pose by differences of rho itself: a rho' that does not belong to rho moves the minimum and shows here.  (The minimal
    shapes are left to the next-step test: their minimum is an exact fit, sum |J| |r| omega is 0 there and the ratio 0 / 0.)"""
    worst_ref = worst_host = 0.0
    for case in CASES:
        if case["minimal"]:
            continue
        out, refs = runs[case["name"]], cases.reference_runs(case)
        for b, r in enumerate(refs):
            a, h = _grad_ratio(case, b, r["R"], r["t"]), _grad_ratio(case, b, out.R[b], out.t[b])
            print(f"{case['name']}[{b}]: reference {a:.2e}, host {h:.2e}")
            worst_ref, worst_host = max(worst_ref, a), max(worst_host, h)
    print(f"gradient / sum |J||r|omega: reference's own minima <= {worst_ref:.2e}, host's <= {worst_host:.2e}, bar {100 * worst_ref:.2e}")
    assert worst_host <= 100.0 * worst_ref


# ---- reductions to the least-squares library -------------------------------------------------------------------------------------------

def _same_as(a, b, what):
    assert a.status.tolist() == b.status.tolist() and a.n_live.tolist() == b.n_live.tolist() and a.iters.tolist() == b.iters.tolist(), what
    assert np.abs(a.R - b.R).max() <= 1e-12 and np.abs(a.t - b.t).max() <= 1e-12, what
    assert (np.abs(a.cost - b.cost) <= 1e-12 * np.abs(b.cost)).all(), what


@pytest.mark.parametrize("shape", [(10, 0), (5, 5), (33, 7), (0, 6)])
def test_l2_without_weights_is_the_least_squares_refinement(rb, shape):
    from cvxpnpl_amd import refine

    d, R0, t0, kw = rc.problem(6, shape[0], shape[1], 1.0)
    a = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], loss="l2", max_iters=100, **kw)
    b = refine.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, **kw)
    _same_as(a, b, shape)
    assert (a.status == 0).all() and (a.n_inlier == a.n_live).all() and (a.robust_w == 1.0).all()


def test_l2_with_weights_zero_and_one_is_the_masked_least_squares_refinement(rb):
    from cvxpnpl_amd import refine

    d, R0, t0, kw = rc.problem(6, 9, 7, 1.0, seed=13)
    masks = rc.boundary_masks(9, 7, 6)
    a = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], loss="l2", max_iters=100, weights_pts=masks["mask_pts"].astype(np.float64),
                                         weights_lines=masks["mask_lines"].astype(np.float64), **kw)
    b = refine.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, **masks, **kw)
    _same_as(a, b, "weights {0, 1}")
    keep = np.concatenate([masks["mask_pts"], masks["mask_lines"]], 1)
    assert (a.robust_w == keep).all() and (a.n_live == keep.sum(1)).all()


def test_huber_with_delta_beyond_every_residual_is_l2(rb, runs):
    case = cases.huge_delta()
    a = runs[case["name"]]
    b = run_host(rb, dict(case, loss="l2"))
    _same_as(a, b, "huge delta")
    assert a.R.tobytes() == b.R.tobytes() and a.cost.tobytes() == b.cost.tobytes()          # the same branch of the same code
    assert (a.robust_w == 1.0).all() and (a.n_inlier == a.n_live).all()


# ---- weights ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", rr.LOSSES)
def test_doubling_all_weights_keeps_the_pose_and_doubles_the_cost(rb, loss):
    case = cases.clean(5, 5, "cauchy")                                                    # (the case with random weights)
    kw = case["kw"]
    a = run_host(rb, dict(case, loss=loss))
    b = run_host(rb, dict(case, loss=loss, kw=dict(kw, weights_pts=2.0 * kw["weights_pts"], weights_lines=2.0 * kw["weights_lines"])))
    assert a.status.tolist() == b.status.tolist() == [0, 0]
    assert np.abs(a.R - b.R).max() <= 1e-12 and np.abs(a.t - b.t).max() <= 1e-12
    assert (np.abs(b.cost - 2.0 * a.cost) <= 1e-12 * np.abs(b.cost)).all()
    assert np.abs(a.robust_w - b.robust_w).max() <= 1e-12


@pytest.mark.parametrize("loss", rr.LOSSES)
def test_zero_weight_on_spoiled_records_is_the_compacted_problem_byte_for_byte(rb, loss):
    d, R0, t0, kw = rc.problem(5, 9, 7, 1.0, seed=17)
    masks = rc.boundary_masks(9, 7, 5)
    rs = np.random.RandomState(5)
    wp, wl = rs.uniform(0.1, 2.0, (5, 9)) * masks["mask_pts"], rs.uniform(0.1, 2.0, (5, 7)) * masks["mask_lines"]
    spoiled, small = rc.spoil_masked(kw, masks), rc.compacted(kw, masks)
    kp, kl = masks["mask_pts"][0] != 0, masks["mask_lines"][0] != 0
    a = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], loss=loss, scale_px=1.5, max_iters=100, weights_pts=wp, weights_lines=wl, **spoiled)
    b = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], loss=loss, scale_px=1.5, max_iters=100, weights_pts=np.ascontiguousarray(wp[:, kp]),
                                         weights_lines=np.ascontiguousarray(wl[:, kl]), **small)
    assert (a.status <= 1).all()
    for f in ("R", "t", "cost", "iters", "status", "n_live", "n_inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    keep = np.concatenate([kp, kl])
    assert a.robust_w[:, keep].tobytes() == b.robust_w.tobytes() and (a.robust_w[:, ~keep] == 0.0).all()


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, -0.0 - 1e-300])
def test_unusable_weight_on_an_admitted_record_is_status_4_and_passes_through(rb, bad):
    d, R0, t0, kw = rc.problem(4, 6, 4, 1.0, seed=19)
    wp, wl = np.ones((4, 6)), np.ones((4, 4))
    wp[1, 2] = bad                                              # admitted: status 4
    wl[2, 3] = bad
    mp = np.ones((4, 6), np.uint8)
    wp[3, 0] = bad                                              # ... behind a zero mask byte: never read
    mp[3, 0] = 0
    out = rb.refine_pose_batch_robust_host(R0, t0, K=d["K"], weights_pts=wp, weights_lines=wl, mask_pts=mp, max_iters=100, **kw)
    assert out.status.tolist() == [0, 4, 4, 0]
    r = rr.refine(d["K"], R0[1], t0[1], weights_pts=wp[1], weights_lines=wl[1], **rc.one(kw, 1))
    assert r["status"] == 4
    for b in (1, 2):
        assert out.R[b].tobytes() == R0[b].tobytes() and out.t[b].tobytes() == t0[b].tobytes()
        assert np.isnan(out.cost[b]).all() and out.iters[b] == 0 and np.isnan(out.robust_w[b]).all() and out.n_inlier[b] == 0
    assert out.n_live[3] == 9 and out.robust_w[3, 0] == 0.0


# ---- the contaminated cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_contaminated_problems_end_at_the_references_robust_minimum(runs, loss):
    case = cases.contaminated_checked()[loss]
    out, refs = runs[case["name"]], cases.reference_runs(case)
    l2 = cases.reference_runs(cases.contaminated("l2"))
    for b, r in enumerate(refs):
        err = max(np.abs(out.R[b] - r["R"]).max(), np.abs(out.t[b] - r["t"]).max())
        far = cases.pose_distance(l2[b]["R"], l2[b]["t"], case["R_gt"][b], case["t_gt"][b])
        near = cases.pose_distance(out.R[b], out.t[b], case["R_gt"][b], case["t_gt"][b])
        print(f"{loss}[{b}]: host - reference's minimum {err:.1e}; from the truth {near:.1e} (the L2 minimum: {far:.1e})")
        assert err <= 1e-8
        assert (out.robust_w[b][case["displaced"][b]] < 0.5).all() and (out.robust_w[b][~case["displaced"][b]] > 0.5).all()


# ---- pass-through ----------------------------------------------------------------------------------------------------------------------

def test_max_iters_0_passes_the_pose_through_bit_for_bit(rb):
    case = cases.clean(5, 5, "cauchy")
    out = run_host(rb, case, max_iters=0)
    assert out.status.tolist() == [1, 1] and out.iters.tolist() == [0, 0]
    assert out.R.tobytes() == case["R0"].tobytes() and out.t.tobytes() == case["t0"].tobytes()
    assert (out.cost[:, 0] == out.cost[:, 1]).all() and np.isfinite(out.cost).all()
    for b in range(2):                                          # the weights are those of the input pose
        w, n_in, _ = rr.robust_w_full(case["K"][b], case["R0"][b], case["t0"][b], "cauchy", case["delta"], **cases.one(case, b))
        assert np.abs(out.robust_w[b] - w).max() <= 1e-9 and out.n_inlier[b] == n_in


@pytest.mark.parametrize("loss", rr.LOSSES)
def test_statuses_2_to_4_pass_through_with_nan_weights(rb, loss):
    K, R0, t0, kw, status_in, masks, expect = rc.edge_batch()
    out = rb.refine_pose_batch_robust_host(R0, t0, K=K, status=status_in, loss=loss, scale_px=2.0, max_iters=100, **masks, **kw)
    assert out.status.tolist() == expect.tolist()
    n_live = np.full(12, 12)
    n_live[5], n_live[7] = 2, 11
    assert out.n_live.tolist() == n_live.tolist()
    for b in range(12):
        if expect[b] >= 2:
            assert out.R[b].tobytes() == R0[b].tobytes() and out.t[b].tobytes() == t0[b].tobytes(), b
            assert np.isnan(out.cost[b]).all() and out.iters[b] == 0 and np.isnan(out.robust_w[b]).all() and out.n_inlier[b] == 0, b
        else:
            assert np.isfinite(out.R[b]).all() and np.isfinite(out.robust_w[b]).all() and out.cost[b, 1] <= out.cost[b, 0], b
            r = rr.refine(K, R0[b], t0[b], loss=loss, delta=2.0, max_iters=100, **rc.one(kw, b, **{k: v[b] for k, v in masks.items()}))
            assert r["status"] == out.status[b] and r["n_live"] == out.n_live[b], b
    assert out.robust_w[7, 8 + 1] == 0.0                         # the degenerate 2D line of problem 7: not live


def test_outputs_may_alias_the_inputs_through_the_c_abi(rb):
    from cvxpnpl_amd import _lib

    case = cases.contaminated("huber")
    want = run_host(rb, case)
    B, kw = len(case["R0"]), case["kw"]
    R, t = case["R0"].copy(), case["t0"].copy()
    cost, iters, st, n_live, n_in = np.empty((B, 2)), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    o = _lib.RefineRobustOpts(C.sizeof(_lib.RefineRobustOpts), cases.MAX_ITERS, 1e-10, 1e-3, _lib.LOSS_HUBER, case["delta"])
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc_ = _lib.refine_robust_lib().cvxpnpl_refine_robust_batch_host(
        B, 20, p(kw["pts_2d"]), p(kw["pts_3d"]), 10, p(kw["line_2d"]), p(kw["line_3d"]), p(case["K"]), 1, p(R), p(t), None, 1, 0x5, None, None, None, None,
        C.byref(o), p(R), p(t), p(cost), p(iters), p(st), p(n_live), None, p(n_in), 2)
    assert rc_ == 0
    assert R.tobytes() == want.R.tobytes() and t.tobytes() == want.t.tobytes() and cost.tobytes() == want.cost.tobytes()
    assert n_in.tolist() == want.n_inlier.tolist() and st.tolist() == want.status.tolist()


def test_threads_and_a_shared_camera_change_nothing(rb):
    case = cases.contaminated("cauchy")
    a = run_host(rb, case, n_threads=1)
    b = rb.refine_pose_batch_robust_host(case["R0"], case["t0"], K=case["K"][0], loss="cauchy", scale_px=case["delta"], max_iters=cases.MAX_ITERS,
                                         n_threads=3, **case["kw"])
    for f in ("R", "t", "cost", "iters", "robust_w", "n_inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
