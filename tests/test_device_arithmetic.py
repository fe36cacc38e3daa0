"""The references the device arithmetic tests (tests/test_device_arithmetic_gpu.py) hold the device branches of csrc/solver_core.h,
quad_kernel.h and wave_kernel.h against, checked on the CPU: the numpy emulation of the rotation branches meets the claims the
headers make, the arguments cover what the callers produce, the domain of the guarded single-precision half-angle is the callers'
domain, and the host instantiations the device figures are compared with meet their own bounds.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_arithmetic_cases as cases  # noqa: E402
import hostsim  # noqa: E402

N_CPU = 300_001  # triples of the CPU tests (the device tests run the full 2 M)


@pytest.fixture(scope="module")
def triples():
    return cases.rotation_arguments(N_CPU)


def test_scalar_arguments_are_the_stated_set():
    x = cases.scalar_arguments()
    assert len(x) == 505 * 2001 and np.isfinite(x).all() and (x > 0).all()
    m, e = np.frexp(x)  # x = m 2^e, m in [0.5, 1)
    assert e.min() == -999 and e.max() == 1001 and len(np.unique(e)) == 2001
    one = x[(e == 1)]  # the binade [1, 2)
    r2 = np.sqrt(cases.ld(2))
    for v in (1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0)):
        assert v in one
    lo, hi = one[one < r2].max(), one[one > r2].min()
    assert hi == np.nextafter(lo, 2.0)  # the two neighbours of sqrt(2)
    assert 2.0 in x and np.nextafter(2.0, 3.0) in x  # 2 and its neighbour above: the first two of the next binade


def test_iterates_stay_inside_the_scale_the_rotation_tests_cover():
    """|W|_F of the iterates the eigen-solves are loaded with (host build, parked after 1 ... 100 iterations) against the range
    [NW_LO, NW_HI] the rotation arguments are drawn from: inside it with a factor 3 to spare at the low end."""
    from cvxpnpl_amd import synth

    wgt = np.array([1.0 if i == j else 2.0 for i in range(10) for j in range(i, 10)])
    lo, hi = np.inf, 0.0
    for n_p, n_l, sigma in ((10, 0, 2.0), (4, 0, 2.0), (0, 6, 1.0)):
        d = synth.make_pnpl(96, n_p, n_l, sigma, seed=3)
        args = (d["pts_2d"] if n_p else None, d["pts_3d"] if n_p else None, d["line_2d"] if n_l else None, d["line_3d"] if n_l else None, d["K"])
        for iters in (1, 3, 10, 100):
            r = hostsim.lane_phase(*args, iters, 0, hostsim.default_opts(first_check=10 ** 6, max_iters=10 ** 6), dbl=True)
            W = r["handoff"][r["status"] == -1, :55]
            nw = np.sqrt((wgt * W * W).sum(1))
            lo, hi = min(lo, nw.min()), max(hi, nw.max())
    print(f"|W|_F of parked iterates: {lo:.3g} ... {hi:.3g} (start iterate: 1)")
    assert 3 * cases.NW_LO <= min(lo, 1.0) and hi * 3 <= cases.NW_HI


# what the headers claim, as bounds on the emulation (300 k triples of the callers' domain).  jacobi_cs(double): "c^2 + s^2 = 1 to rounding"
# (c within 2 ulp of 1 / sqrt(x), squared, and s = t c rounded once more: the 8 ulp of the exact forms), an angle "right to ~1e-7"; the exact float64 forms: "a rotation to the precision of that one root" (rsqrt_: <= 2 ulp, squared and
# summed: 8 ulp), "leaves 1e-7 of the pair's inner product standing", "dl holds for any angle"; single precision: the same in float32 (a
# hardware seed of 1 ulp enters c^2 + s^2 through 1 / h and twice through 1 / c: 16 ulp of float32 cover it).  "~1e-7" is read as < 1e-6.
CLAIMS = {
    "jacobi_cs": {"unit": 8 * 2.0 ** -52, "resid": 1e-6, "update": 1e-6, "outer": 1e-6},
    "jacobi_cs_dl": {"unit": 8 * 2.0 ** -52, "resid": 1e-6, "update": 1e-6, "outer": 1e-6},
    "jacobi_cs_dl_exact": {"unit": 8 * 2.0 ** -52, "resid": 1e-6, "update": 8 * 2.0 ** -52, "outer": 1e-6},
    "pair_cs_f64": {"unit": 8 * 2.0 ** -52, "resid": 1e-6, "update": 8 * 2.0 ** -52, "outer": 1e-6},
    "jacobi_cs_f32": {"unit": 16 * 2.0 ** -24, "resid": 1e-6, "update": 1e-6, "outer": 1e-6},
    "pair_cs": {"unit": 16 * 2.0 ** -24, "resid": 1e-6, "update": 1e-6, "outer": 1e-6},
}


def emulated_metrics(name, unit, al, be, gam, ulps=1):
    a, rot, tie, d, apb = cases.rotation_case(name, al, be, gam)
    c, s, u = cases.emulate(name, a, rot, tie, unit, ulps)
    k = rot & (np.asarray(a[-1]) != 0)
    return cases.rotation_metrics(name, d[k], np.asarray(a[-1])[k], apb[k], c[k], s[k], u[k]), rot


# (the quad kernel's forms exist in the solver library's unit only)
BRANCHES = [(n, u) for n in sorted(CLAIMS) for u in ("c3", "newton2") if not (u == "newton2" and n.startswith("pair_cs"))]


@pytest.mark.parametrize("name,unit", BRANCHES)
def test_emulation_meets_the_documented_claims(triples, name, unit):
    """The numpy emulation of each device branch (device_arithmetic_cases.emulate: hardware seeds moved by one ulp either way) on the
    callers' domain, held to what the comments in solver_core.h and quad_kernel.h say of the branch.  (outer: how far |s| may exceed c.
    Every form divides by a rounded root, so at d = 0 it reaches |s| = c (1 +- the error of that root: a single-precision seed in all
    but the exact forms, the raw float64 seed of h in those) -- 45 degrees from either side, the same rotation to the angle's ~1e-7.)"""
    for ulps in (0, 1):
        m, rot = emulated_metrics(name, unit, *triples, ulps=ulps)
        print(f"emulation {name} [{unit}] seeds +-{ulps} ulp: " + "  ".join(f"{k} {v:.3g}" for k, v in m.items()))
        assert rot.all()  # (|cos| >= 1e-14: every triple of the domain rotates)
        for k, bound in CLAIMS[name].items():
            assert m[k] <= bound, (k, m[k], bound)


def test_emulation_notices_the_defects_the_device_tests_are_there_for():
    """The figures are sharp enough to tell a wrong branch from a right one: a lost refinement step, a wrong sign in dl."""
    al, be, gam = cases.rotation_arguments(50_001)
    a, rot, tie, d, apb = cases.rotation_case("jacobi_cs_dl_exact", al, be, gam)
    c, s, dl = cases.emulate("jacobi_cs_dl_exact", a, rot)
    bad = s * (s * d + c * 2 * gam)  # + in place of -
    m = cases.rotation_metrics("jacobi_cs_dl_exact", d, gam, apb, c, s, bad)
    assert m["update"] > 1e-3
    m = cases.rotation_metrics("jacobi_cs_dl_exact", d, gam, apb, c * (1 + 1e-9), s, dl)  # a root that lost a step
    assert m["unit"] > 4 * CLAIMS["jacobi_cs_dl_exact"]["unit"]


def test_the_guarded_half_angle_is_a_rotation_on_the_callers_domain():
    """jacobi_cs(float) and cvxq::pair_cs add 1e-37 to h2 = d^2 + 4 gam^2 so that rot = false cannot breed a NaN.  Where the guard is
    not small beside h2 the result is no rotation (d = 0, gam -> 0: c -> 0.71, s -> 0: both columns SHRINK).  The domain argument:

      the callers rotate only when gam^2 > 1e-30 al be, and al, be >= (0.5 |W|_F)^2 (device_arithmetic_cases: scale of the arguments),
      so h2 >= 4 gam^2 > 4e-30 (0.25 |W|_F^2)^2 = 2.5e-31 |W|_F^4: a factor 2.5e6 |W|_F^4 above the guard.  |W|_F >= 1 on every iterate
      measured (the start iterate has exactly 1): the guard moves c^2 + s^2 by at most 1 / (2 * 2.5e6) = 2e-7 there, inside the 16 ulp of
      float32 the seeds cost anyway, and only at be == al with gam at 1e-15 of them.  At the low end of what the tests cover (|W|_F = 0.3)
      the factor is 2e4 and the defect 2.5e-5 -- still a rotation to the precision the sweeps need (tolerance 6e-2), and bounded below.

    Outside that domain (|W|_F ~ 1e-2 and smaller: squared norms of 1e-5) it is no rotation.  No caller gets there: sigma = 1.5 |W|_F
    scales the columns, and |W|_F < 0.3 would need an iterate with Z99 far from 1."""
    assert cases.guard_margin(1.0) >= 2.49e6 and cases.guard_margin(cases.NW_LO) >= 2e4
    al, be, gam = cases.boundary_arguments()
    for name in ("jacobi_cs_f32", "pair_cs"):
        a, rot, tie, d, apb = cases.rotation_case(name, al, be, gam)
        assert (d == 0).all() and rot.sum() > 0.6 * len(rot)
        c, s, t = cases.emulate(name, a, rot, tie)
        unit = np.abs(c.astype(cases.ld) ** 2 + s.astype(cases.ld) ** 2 - 1).astype(np.float64)
        assert (unit[rot] <= cases.half_angle_bound(a[-1][rot])).all()
        assert unit[rot].max() <= 0.5 / cases.guard_margin(cases.NW_LO) + 16 * 2.0 ** -24
        assert (c[~rot] == 1).all() and (s[~rot] == 0).all()
    # outside the callers' domain: squared norms of 1e-6 (|W|_F = 1e-3)
    al = np.full(8, 1e-6)
    gam = 1.5 * np.sqrt(cases.ROT_EPS) * al * np.array([1, -1] * 4)
    a, rot, tie, d, apb = cases.rotation_case("jacobi_cs_f32", al, al.copy(), gam)
    c, s, t = cases.emulate("jacobi_cs_f32", a, rot)
    assert rot.all() and (np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1) > 0.4).all()


def test_special_argument_table_host_column():
    """The host branches of rcp / rsqrt_ / sqrt_fast on the special arguments: IEEE, as device_arithmetic_cases.HOST_TABLE says (the
    device column is checked on the device, tests/test_device_arithmetic_gpu.py: test_special_arguments)."""
    for name, row in cases.HOST_TABLE.items():
        with np.errstate(all="ignore"):
            y = hostsim.scalar(name, cases.SPECIALS)
        got = [cases.classify(name, x, v) for x, v in zip(cases.SPECIALS, y)]
        assert got == row, (name, got)


def test_psd_projection_on_the_spectra_the_solver_meets():
    """test_psd_projection_matches_numpy's body (same bounds) on trace-normalised iterates with Z99 = 1, rank 1 plus noise of 1e-9 and a
    ten-fold eigenvalue, host build."""
    cases.check_psd_projection_matches_numpy(hostsim, cases.solver_spectra())


def test_single_precision_eigen_solve_host_instantiation():
    """cvx::EigF on the host (hs_pospart_f32) against numpy.linalg.eigh: single-precision columns of G = W + sigma I with sigma = 1.5 |W|_F
    resolve the eigenvalues to a few float32 ulp of 2.5 |W|_F -- the figure the device instantiation is held to 4x of."""
    worst = 0.0
    for M in cases.psd_projection_matrices() + cases.solver_spectra():
        w, v = np.linalg.eigh(M)
        Wp, lam, sweeps = hostsim.pospart_f32(cases.pack55(M))
        nrm = np.linalg.norm(M)
        worst = max(worst, np.abs(np.sort(lam) - w).max() / nrm, np.abs(cases.unpack55(Wp) - (v * np.maximum(w, 0)) @ v.T).max() / nrm)
        assert sweeps <= 30
    print(f"EigF host: worst error / |W|_F {worst:.3g}")
    assert worst < 64 * 2.0 ** -24 * 2.5  # (64 ulp of the largest shifted eigenvalue: ten columns, a few sweeps)


def test_polar_factor_host_build():
    M, cond = cases.polar_inputs()
    ref = cases.polar_reference(M)
    R = hostsim.polar3_batch(M, 40)
    err = np.abs(R - ref).max(axis=(1, 2))
    print(f"polar3 host: worst |R - U Vh| / (eps cond) {(err / (2.0 ** -52 * cond)).max():.3g}")
    assert (err <= cases.POLAR_C * 2.0 ** -52 * cond).all()
    near = cond < 2
    R8 = hostsim.polar3_batch(M[near], 8)  # (round_candidate's count, on what it is given: near-rotations)
    assert (np.abs(R8 - ref[near]).max(axis=(1, 2)) <= cases.POLAR_C * 2.0 ** -52 * cond[near]).all()
    assert (np.sign(np.linalg.det(R)) == np.sign(np.linalg.det(M))).all()  # reflections are preserved
    Mi, det = hostsim.inv3_batch(M)
    # (cofactors: products of size s1^2 with rounding errors of eps s1^2, against det = s1 s2 s3 -- relative eps s1^2 / (s2 s3) <= eps cond^2)
    assert (np.abs(det / np.linalg.det(M) - 1) <= cases.INV3_C * 2.0 ** -52 * cond ** 2).all()
    assert (np.abs(Mi @ M - np.eye(3)).max(axis=(1, 2)) <= cases.INV3_C * 2.0 ** -52 * cond ** 2).all()
    Rn = hostsim.near_rotation_batch(M[near])
    assert np.abs(Rn.transpose(0, 2, 1) @ Rn - np.eye(3)).max() < 16 * 2.0 ** -52  # orthogonal to rounding: what the polish needs


@pytest.mark.slow
def test_devsim_compiles_for_gfx950_with_the_products_flags(tmp_path):
    """tests/devsim cross-compiles without a GPU: catches a header (solver_core.h, quad_kernel.h, wave_kernel.h) that no longer
    includes stand-alone, in either unit, with the flags of cvxpnpl_amd/build.py: compile_cmd()."""
    import devsim
    from cvxpnpl_amd.build import compile_cmd

    for flag in ("--offload-arch=gfx950", "-O3", "-std=c++17", "-enable-ipra=0"):
        assert flag in compile_cmd() and flag in devsim.unit_cmd("x.hip", "x.o")
    assert not any(f.startswith("-ffp-contract") for f in devsim.unit_cmd("x.hip", "x.o"))
    out = devsim.build(force=True, out=str(tmp_path / "libdevsim_check.so"))
    assert os.path.getsize(out) > 0
