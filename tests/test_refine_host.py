"""cvxpnpl_refine_batch_host (the source of the refinement kernels, on host threads) against the independent numpy reference
(tests/refine_reference.py).  No GPU needed.

Measured on the six shapes (batch 24, start 0.05 rad and 5 % of t off the truth): every problem converges within 7 trials; the reference's
next step from the returned poses is at most 1e-8 (bar 1e-6); the covariance deviates by at most 0.02 of its bound; the noise-free case
ends at rms 2e-13 px and 2e-15 rad from the truth; a second call converges on its first trial."""
import numpy as np
import pytest

import refine_cases as rc
import refine_reference as ref
from cvxpnpl_amd import synth

B = 24


@pytest.fixture(scope="module")
def rf():
    from cvxpnpl_amd import build, refine

    build.build_refine()
    return refine


@pytest.fixture(scope="module")
def runs(rf):
    """Each shape refined once (max_iters = 100, with covariance), shared by the tests below."""
    out = {}
    for n_p, n_l, sigma in rc.SHAPES:
        d, R0, t0, kw = rc.problem(B, n_p, n_l, sigma)
        out[(n_p, n_l)] = (d, R0, t0, kw, rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, **kw))
    return out


@pytest.mark.parametrize("shape", [s[:2] for s in rc.SHAPES])
def test_converges_monotone_orthonormal_and_stationary(runs, shape):
    d, R0, t0, kw, out = runs[shape]
    assert (out.status == 0).all(), out.status
    assert (out.n_live == shape[0] + shape[1]).all()
    assert (out.cost[:, 1] <= out.cost[:, 0]).all()                                     # exact
    assert np.abs(np.swapaxes(out.R, 1, 2) @ out.R - np.eye(3)).max() <= 1e-13
    assert (np.linalg.det(out.R) > 0).all()
    worst = rc.worst_next_step(d["K"], out.R, out.t, kw)
    print(f"{shape}: iters <= {out.iters.max()}, reference's next step <= {worst:.2e}")
    assert worst <= rc.STEP_BAR


def test_agrees_with_the_reference_schedule(rf):
    """The reference runs the same schedule in the public chart with a finite-difference Jacobian: same minimum, same cost."""
    d, R0, t0, kw = rc.problem(4, 10, 0, 1.0)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, **kw)
    for b in range(4):
        r = ref.refine(d["K"], R0[b], t0[b], max_iters=100, **rc.one(kw, b))
        assert r["status"] == 0 and all(x >= y for x, y in zip(r["history"], r["history"][1:]))     # the reference's cost never increases
        assert abs(r["cost"][0] - out.cost[b, 0]) <= 1e-9 * r["cost"][0] and abs(r["cost"][1] - out.cost[b, 1]) <= 1e-9 * r["cost"][1]
        assert np.abs(r["R"] - out.R[b]).max() <= rc.STEP_BAR and np.abs(r["t"] - out.t[b]).max() <= rc.STEP_BAR


def test_noise_free_reaches_the_truth(rf):
    d, R0, t0, kw = rc.problem(B, 10, 0, 0.0)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, **kw)
    assert (out.status == 0).all()
    rms = np.sqrt(out.cost[:, 1] / 20.0)
    geo = synth.geodesic(out.R, d["R_gt"])
    print(f"noise-free: rms <= {rms.max():.1e} px, geodesic <= {geo.max():.1e} rad")
    assert rms.max() <= 1e-8 and geo.max() <= 1e-10


@pytest.mark.parametrize("shape", [(10, 0), (5, 5)])
@pytest.mark.parametrize("sigma_px", [0.0, 1.5])
def test_covariance(rf, runs, shape, sigma_px):
    d, R0, t0, kw, out = runs[shape]
    if sigma_px > 0:
        out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, sigma_px=sigma_px, **kw)
    assert np.abs(out.cov - np.swapaxes(out.cov, 1, 2)).max() <= 1e-12 * np.abs(out.cov).max()
    worst = rc.worst_cov_ratio(d["K"], out, kw, sigma_px)
    print(f"{shape} sigma_px={sigma_px}: covariance error / bound <= {worst:.3f}")
    assert worst <= 1.0


def test_covariance_needs_more_than_six_residuals(rf):
    d, R0, t0, kw = rc.problem(4, 3, 0, 0.0)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, **kw)
    assert (out.status <= 1).all() and np.isnan(out.cov).all()                         # m = 6: no sigma^2 from the residuals
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], max_iters=100, want_cov=True, sigma_px=1.0, **kw)
    assert np.isfinite(out.cov[out.status <= 1]).all()


@pytest.mark.parametrize("shape", [s[:2] for s in rc.SHAPES])
def test_idempotent(rf, runs, shape):
    d, R0, t0, kw, out = runs[shape]
    again = rf.refine_pose_batch_host(out.R, out.t, K=d["K"], max_iters=100, **kw)
    assert (again.status == 0).all() and again.iters.max() <= 2, (again.status, again.iters)
    assert (again.cost[:, 1] <= again.cost[:, 0]).all() and np.abs(again.cost[:, 0] - out.cost[:, 1]).max() <= 1e-12 * out.cost[:, 1].max()


def test_edge_cases_pass_through_bit_for_bit(rf):
    K, R0, t0, kw, status_in, masks, expect = rc.edge_batch()
    out = rf.refine_pose_batch_host(R0, t0, K=K, status=status_in, max_iters=100, want_cov=True, **masks, **kw)
    rc.check_edge_batch(out, R0, t0, expect)
    live = np.nonzero(expect < 2)[0]
    assert rc.worst_next_step(K, out.R, out.t, kw, rows=live, masks=masks) <= rc.STEP_BAR


def test_masked_records_never_reach_the_output(rf):
    d, R0, t0, kw = rc.problem(6, 12, 0, 1.0, seed=5)
    keep = np.ones(12, bool)
    keep[[1, 4, 7, 10]] = False
    mask = np.tile(keep.astype(np.uint8), (6, 1))
    p2, p3 = kw["pts_2d"].copy(), kw["pts_3d"].copy()
    p2[:, ~keep] = np.nan
    p3[:, ~keep] = 1e9
    p3[:, 1] = np.nan
    a = rf.refine_pose_batch_host(R0, t0, pts_2d=p2, pts_3d=p3, K=d["K"], mask_pts=mask, max_iters=100, want_cov=True)
    b = rf.refine_pose_batch_host(R0, t0, pts_2d=np.ascontiguousarray(kw["pts_2d"][:, keep]), pts_3d=np.ascontiguousarray(kw["pts_3d"][:, keep]),
                                  K=d["K"], max_iters=100, want_cov=True)
    assert (a.status == 0).all() and (b.status == 0).all() and (a.n_live == 8).all()
    assert np.isfinite(a.R).all() and np.isfinite(a.t).all() and np.isfinite(a.cost).all() and np.isfinite(a.cov).all()
    worst = max(np.abs(a.R - b.R).max(), np.abs(a.t - b.t).max())
    print(f"masked against compacted: {worst:.2e}")
    assert worst <= rc.STEP_BAR


def test_minimal_shape_stays_sane(rf):
    d, R0, t0, kw = rc.problem(B, 3, 1, 1.0)
    out = rf.refine_pose_batch_host(R0, t0, K=d["K"], **kw)                             # the default 30 trials
    assert np.isfinite(out.R).all() and np.isfinite(out.t).all() and np.isfinite(out.cost).all()
    assert (out.cost[:, 1] <= out.cost[:, 0]).all() and np.isin(out.status, (0, 1)).all()


def test_per_problem_K_and_threads(rf):
    d, R0, t0, kw = rc.problem(9, 5, 5, 1.0)
    Kb = np.tile(d["K"], (9, 1, 1))
    a = rf.refine_pose_batch_host(R0, t0, K=d["K"], n_threads=1, **kw)
    b = rf.refine_pose_batch_host(R0, t0, K=Kb, n_threads=4, **kw)
    assert a.R.tobytes() == b.R.tobytes() and a.cost.tobytes() == b.cost.tobytes() and a.iters.tolist() == b.iters.tolist()
