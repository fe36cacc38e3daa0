"""The host twin of the pose VJP (cvxpnpl_pose_vjp_host; vjp_core.h, the source of the kernels) against an independent float64
autograd reference (grad_reference.reference_vjp: the cost's definition, torch.matrix_exp, double backward) -- no GPU, no oracle.

Poses: the ground truth polished by the test's own Gauss-Newton until |g| is at rounding level; whole small batches are checked.
Truth: the reference in the chart centred on the 3D records.  The same reference in the plain chart (centre 0) is correct at a
stationary pose too; its disagreement with the truth is the reference's own noise floor and is held below the bound as well.

Error: relative L2 per problem over all four gradients.  Measured over the cases below (every problem of every case, the reflected
poses included): worst host-vs-reference error 2.45e-13 (pnp10-far; 1.9e-13 for pnl3, below 7e-14 away from the far-origin and
minimal cases), worst floor 8.6e-11 for the far-origin scenes in the plain chart and 1.1e-13 for every other case.
BOUND = 2.5e-11 = 100 x the worst error: the error grows with cond(H), which varies by two orders across seeds.  The floor is
asserted below 1e-9 for the far-origin scenes (the plain chart loses |c|^2 / spread^2 ~ 1e4 digits there, which is why the product
centres its chart and why the centred reference is the truth) and below BOUND elsewhere.

A problem counts as polished when polish's |g| / (2 |J| |r|) is below 1e-12 -- or when the pose fits the data exactly (noise-free
data, the minimal problems n = 3: |r| below 1e-13 of its terms), where g = 2 J^T r vanishes with r and that ratio is 0 / 0.  At
most 5 % of a case may fail to polish; with these seeds none does.

What the test catches (mutants of vjp_core.h, tried by hand; DESIGN.md section 11 has the table): a Gauss-Newton H, a missing
normalisation term of the line normal, a 1e-8 relative error in the second-order sums and a flipped sign of the translation
coupling in b all fail here; a different chart centre does not, and must not.
"""
import numpy as np
import pytest

import grad_reference as gr
from cvxpnpl_amd import synth
from cvxpnpl_amd.grad import ADMIT_CERTIFIED, ADMIT_RANK1, pose_vjp_host

BOUND = 2.5e-11
FLOOR_FAR = 1e-9
K_GENERAL = np.array([[510.0, 2.5, 301.0], [0.0, 540.0, 262.0], [0.0, 0.0, 1.0]])
FAR_A, FAR_B = np.array([40.0, -25.0, 60.0]), np.array([-30.0, 45.0, 20.0])

# name: (n_p, n_l, batch, seed, options)
CASES = {
    "pnp3": (3, 0, 8, 101, {}), "pnp4": (4, 0, 8, 102, {}), "pnp6": (6, 0, 8, 103, {}), "pnp10": (10, 0, 8, 104, {}),
    "pnp50": (50, 0, 8, 105, {}), "pnp900": (900, 0, 3, 106, {}),
    "pnl3": (0, 3, 8, 307, {}), "pnl6": (0, 6, 8, 108, {}), "pnl10": (0, 10, 8, 109, {}), "pnl400": (0, 400, 3, 110, {}),
    "pnpl5+5": (5, 5, 8, 111, {}), "pnpl1+3": (1, 3, 8, 112, {}), "pnpl300+300": (300, 300, 3, 113, {}),
    "pnp10-Kgeneral": (10, 0, 8, 114, {"K": K_GENERAL}), "pnpl5+5-Kgeneral": (5, 5, 8, 115, {"K": K_GENERAL}),
    "pnp10-Kper": (10, 0, 8, 116, {"K_per": True}), "pnpl5+5-Kper": (5, 5, 8, 117, {"K_per": True}),
    "pnp10-far": (10, 0, 8, 118, {"far": FAR_A}), "pnpl5+5-far": (5, 5, 8, 119, {"far": FAR_B}),
    "pnp10-first-record-far": (10, 0, 8, 120, {"outlier": True}), "pnl6-first-record-far": (0, 6, 8, 121, {"outlier": True}),
    "pnp10-sigma0": (10, 0, 8, 122, {"sigma": 0.0}), "pnpl5+5-sigma0": (5, 5, 8, 123, {"sigma": 0.0}),
}
# (pnl3: a noisy minimal line problem often has no exact real solution near the truth, and Gauss-Newton from the ground truth then stalls
# far from stationary -- for about one problem in five; this seed is one where all eight polish.)
REFLECTED = ("pnp4", "pnp10", "pnl6", "pnpl5+5", "pnpl300+300", "pnp10-Kper", "pnpl5+5-far")


def make_case(name):
    n_p, n_l, batch, seed, opt = CASES[name]
    sigma = opt.get("sigma", 2.0)
    d = synth.make_pnpl(batch, n_p, n_l, sigma=sigma, seed=seed, K=opt.get("K", synth.K_KINECT))
    if opt.get("outlier"):  # the first 3D record far from the rest of the scene, seen where it is (its pixel noise drawn again)
        key3, key2 = ("pts_3d", "pts_2d") if n_p else ("line_3d", "line_2d")
        P = d[key3].reshape(batch, -1, 3)
        P[:, 0] *= 10.0  # ten scene radii away.  (Further out the test's own polish, centred on the dragged mean, stops short of 1e-12.)
        x = synth.project(P[:, :1], d["K"], d["R_gt"], d["t_gt"]) + np.random.RandomState(seed).normal(scale=sigma, size=(batch, 1, 2))
        d[key2].reshape(batch, -1, 2)[:, 0] = x[:, 0]
    if opt.get("K_per"):
        d = gr.per_problem_K(d, seed)
    if "far" in opt:  # the same images, the world origin moved far from the scene
        d["pts_3d"] = d["pts_3d"] + opt["far"]
        d["line_3d"] = d["line_3d"] + opt["far"]
        d["t_gt"] = d["t_gt"] - d["R_gt"] @ opt["far"]
    return d


def polished(d, name):
    R, t, g, fit = gr.polish_batch(d)
    good = (g < 1e-12) | (fit < 1e-13)
    assert (~good).sum() <= 0.05 * len(g), (name, g, fit)
    return R, t, good


def check_against_reference(name, d, R, t, good, GR, gt, out, floor_bound):
    worst = worst_floor = 0.0
    for b in np.flatnonzero(good):
        assert out["vjp_status"][b] == 0, (name, b, out["vjp_status"])
        truth, floor = gr.reference_truth_and_floor(R[b], t[b], *gr.problem(d, b), GR[b], gt[b])
        err = gr.rel_err(gr.flat(out, b), truth)
        worst, worst_floor = max(worst, err), max(worst_floor, floor)
    print(f"{name}: {good.sum()} problems, worst host-vs-reference {worst:.2e}, worst floor (plain chart) {worst_floor:.2e}")
    assert worst < BOUND, (name, worst)
    assert worst_floor < floor_bound, (name, worst_floor)


@pytest.mark.parametrize("name", list(CASES))
def test_host_vjp_matches_the_autograd_reference(name):
    d = make_case(name)
    batch = d["R_gt"].shape[0]
    R, t, good = polished(d, name)
    rng = np.random.default_rng(CASES[name][3])
    GR, gt = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
    out = pose_vjp_host(R, t, np.zeros(batch, np.int32), GR, gt, K=d["K"], **gr.kinds(d))
    check_against_reference(name, d, R, t, good, GR, gt, out, FLOOR_FAR if "far" in CASES[name][4] else BOUND)


@pytest.mark.parametrize("name", REFLECTED)
def test_reflected_poses_match_the_reference_and_the_sign_identity(name):
    """f is invariant under (R, t) -> (-R, -t): the negated polished pose is a stationary point with det R = -1 (what the solver
    reports as CVXPNPL_REFLECTION and ADMIT_RANK1 admits), and VJP(-R, -t; G_R, g_t) = VJP(R, t; -G_R, -g_t)."""
    d = make_case(name)
    batch = d["R_gt"].shape[0]
    R, t, good = polished(d, name)
    assert (np.linalg.det(-R) < 0).all()
    rng = np.random.default_rng(CASES[name][3] + 1000)
    GR, gt = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
    refl = pose_vjp_host(-R, -t, np.full(batch, 4, np.int32), GR, gt, K=d["K"], admit_mask=ADMIT_RANK1, **gr.kinds(d))
    check_against_reference(name + " reflected", d, -R, -t, good, GR, gt, refl, FLOOR_FAR if "far" in CASES[name][4] else BOUND)
    twin = pose_vjp_host(R, t, np.zeros(batch, np.int32), -GR, -gt, K=d["K"], **gr.kinds(d))
    for b in np.flatnonzero(good):
        assert gr.rel_err(gr.flat(refl, b), gr.flat(twin, b)) < BOUND, (name, b)
    # and a reflection is skipped unless the mask admits it
    skipped = pose_vjp_host(-R, -t, np.full(batch, 4, np.int32), GR, gt, K=d["K"], admit_mask=ADMIT_CERTIFIED, **gr.kinds(d))
    assert (skipped["vjp_status"] == 1).all() and not gr.flat(skipped).any()


@pytest.mark.parametrize("name", ["pnp10", "pnpl5+5"])
def test_absent_upstream_gradients_and_status(name):
    d = make_case(name)
    batch = d["R_gt"].shape[0]
    R, t, good = polished(d, name)
    rng = np.random.default_rng(7)
    GR, gt = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
    kw = dict(K=d["K"], **gr.kinds(d))
    st = np.zeros(batch, np.int32)
    # None is zero: against the reference, and bit for bit against explicit zeros
    only_t = pose_vjp_host(R, t, st, None, gt, **kw)
    check_against_reference(name + " grad_R=None", d, R, t, good, np.zeros_like(GR), gt, only_t, BOUND)
    only_R = pose_vjp_host(R, t, st, GR, None, **kw)
    check_against_reference(name + " grad_t=None", d, R, t, good, GR, np.zeros_like(gt), only_R, BOUND)
    assert np.array_equal(gr.flat(only_t), gr.flat(pose_vjp_host(R, t, st, np.zeros_like(GR), gt, **kw)))
    assert np.array_equal(gr.flat(only_R), gr.flat(pose_vjp_host(R, t, st, GR, np.zeros_like(gt), **kw)))
    # status None: every problem, whatever the mask
    full = pose_vjp_host(R, t, st, GR, gt, **kw)
    for admit in (ADMIT_CERTIFIED, ADMIT_RANK1, 0):
        free = pose_vjp_host(R, t, None, GR, gt, admit_mask=admit, **kw)
        assert np.array_equal(gr.flat(free), gr.flat(full)) and (free["vjp_status"] == 0).all()
        assert np.array_equal(free["info"], full["info"])


def test_thread_count_does_not_change_a_bit():
    d = make_case("pnpl5+5")
    big = synth.make_pnpl(37, 6, 3, sigma=2.0, seed=9)
    for dd in (d, big):
        batch = dd["R_gt"].shape[0]
        rng = np.random.default_rng(3)
        GR, gt = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
        st = (np.arange(batch) % 5).astype(np.int32)
        one = pose_vjp_host(dd["R_gt"], dd["t_gt"], st, GR, gt, K=dd["K"], admit_mask=ADMIT_RANK1, n_threads=1, **gr.kinds(dd))
        for nt in (2, 5, 16, 64, 0):
            many = pose_vjp_host(dd["R_gt"], dd["t_gt"], st, GR, gt, K=dd["K"], admit_mask=ADMIT_RANK1, n_threads=nt, **gr.kinds(dd))
            assert np.array_equal(gr.flat(one), gr.flat(many)) and np.array_equal(one["vjp_status"], many["vjp_status"])
            assert np.array_equal(one["info"], many["info"], equal_nan=True)


UNDERDETERMINED = [(1, 0), (2, 0), (0, 1), (0, 2), (1, 1)]


@pytest.mark.parametrize("n_p,n_l", UNDERDETERMINED, ids=[f"{p}pt+{l}ln" for p, l in UNDERDETERMINED])
def test_fewer_than_six_equations_are_singular(n_p, n_l):
    """A point gives two equations and a line two; fewer than three correspondences determine no pose.  At an exact minimiser
    (noise-free data, the true pose) H is the Gauss-Newton matrix and the pivot test finds its null space.  Away from one (noisy data,
    status None) the second-order term lifts that null space by about the relative residual, ~1e-4, far above the pivot tolerance:
    1 point + 1 line used to come back VJP_OK for a quarter of such problems.  Decision: that was a bug -- no v exists -- and
    solve_v now reports VJP_SINGULAR from the count alone (vjp_core.h, include/cvxpnpl_amd_grad.h)."""
    for sigma in (0.0, 2.0):
        d = synth.make_pnpl(8, n_p, n_l, sigma=sigma, seed=50 + n_p + 3 * n_l)
        rng = np.random.default_rng(1)
        out = pose_vjp_host(d["R_gt"], d["t_gt"], None, rng.standard_normal((8, 3, 3)), rng.standard_normal((8, 3)), K=d["K"], **gr.kinds(d))
        assert (out["vjp_status"] == 2).all(), (sigma, out["vjp_status"])
        assert not gr.flat(out).any()
    # three correspondences are enough
    d = synth.make_pnpl(8, 2 if n_p else 0, 3 - (2 if n_p else 0), sigma=0.0, seed=60)
    out = pose_vjp_host(d["R_gt"], d["t_gt"], None, np.ones((8, 3, 3)), np.ones((8, 3)), K=d["K"], **gr.kinds(d))
    assert (out["vjp_status"] == 0).all()
