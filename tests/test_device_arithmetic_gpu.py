"""The device side of csrc/solver_core.h, quad_kernel.h and wave_kernel.h on its own: the `#if defined(__HIP_DEVICE_COMPILE__)` branches
(hardware seeds plus hand-written refinement in place of IEEE divide and sqrt) and the rest of the headers as hipcc's device pass
compiles them (FMA contraction), through the probe kernels of tests/devsim, against long-double references, the numpy emulation of
the branches (tests/device_arithmetic_cases.py, itself held to the headers' claims by tests/test_device_arithmetic.py) and the bounds
of the host tests.  Both translation units: "c3" (the solver library's) and "newton2" (lane_kernel.hip's, CVX_REFINE_NEWTON2).
Run with -s for one line of worst values per function and unit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_arithmetic_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
UNITS = ("c3", "newton2")


@pytest.fixture(scope="module")
def dev():
    import torch

    from cvxpnpl_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    import devsim

    devsim.lib()
    return devsim


# ------------------------------------------------------------------------------------------------------------------------------
# scalar primitives

SCALARS = [(n, u) for n in ("rcp", "rsqrt_", "sqrt_fast") for u in UNITS] + [("fast_rcp", "c3")]


@pytest.fixture(scope="module")
def scalar_refs():
    x = cases.scalar_arguments()
    return x, {n: cases.scalar_reference(n, x) for n in ("rcp", "rsqrt_", "sqrt_fast")}


@pytest.mark.parametrize("name,unit", SCALARS)
def test_scalar_primitives_within_two_ulp(dev, scalar_refs, name, unit):
    """rcp, rsqrt_, sqrt_fast (both units) and cvxw::fast_rcp against long double 1 / x, 1 / sqrt(x), sqrt(x) on every binade from
    2^-1000 to 2^1000 (device_arithmetic_cases.scalar_arguments; both signs for the reciprocals): relative error <= 2^-51, the
    header's "<= 1-2 ulp".  (The project's own figure, 1.38e-16 for rsqrt_, was measured over 1e-12 ... 1e12 only.)"""
    x, refs = scalar_refs
    ref = refs["rcp" if name == "fast_rcp" else name]
    err = cases.rel_err(dev.scalar(name, x, unit), ref)
    worst, at = err.max(), x[err.argmax()]
    if name in ("rcp", "fast_rcp"):
        en = cases.rel_err(dev.scalar(name, -x, unit), -ref)
        if en.max() > worst:
            worst, at = en.max(), -x[en.argmax()]
    print(f"\n{name} [{unit}]: worst relative error {worst:.3e} = {worst * 2.0 ** 52:.2f} ulp at x = {at!r} ({len(x)} arguments)")
    assert worst <= cases.ULP2


def test_special_arguments(dev):
    """+-0, +-inf, NaN, negatives, subnormals and |x| > 2^1000: what the device branches return (device_arithmetic_cases.SPECIAL_TABLE,
    the table in the comment above cvx::rcp) beside the host branches (HOST_TABLE, checked on the CPU).  They differ by construction: the
    refinement step multiplies 0 by inf (rcp(0): r = inf, e = fma(-0, inf, 1) = NaN; rcp(inf): r = 0, e = fma(-inf, 0, 1) = NaN;
    rsqrt_(0): y = inf, x y = NaN), so the device returns NaN where IEEE returns inf or 0, and sqrt_fast's `x > 0 ? ... : 0` turns NaN and
    negatives into 0 where sqrt returns NaN.

    Can such an argument reach a call site, and what guards it (wave_kernel.h, quad_kernel.h, assemble_kernel.h, ipm_wave.h)?
      rcp(det) in inv3 <- assemble / gram_finish (K, N^T N): det = 0 or NaN for a singular K or fewer than two distinct bearings.
        Device NaN, host inf; guarded AFTER the call: `det == det && det != 0` (assemble) and `!(det > 1e-12 scale^3 / 27)` (gram_finish)
        reject both, the problem is ST_NONFINITE in either build.  Also <- polar3 (singular X, below: test_polar_factors).
      rcp(tr) (the trace normalisation of the wave and quad kernels): guarded before, `finite ? rcp(tr) : 0` with finite = tr > 0 && tr < 1e300.  tr subnormal is not
        excluded: rcp is NaN there (host inf), Qs non-finite either way -> ST_NONFINITE in both builds.
      rcp(v[9]) (cvxw::coop_round, cvx::rounds_to): v[9] = 0 only for a top eigenvector with an exactly zero last entry; device NaN, host
        inf: M0 is non-finite in both, d0 > 0 fails in both (inf - inf = NaN in det3), the candidate is dropped.
      rcp(al), rsqrt_(al), sqrt_fast(al) (positive part, warm start and top eigenvectors of the wave and quad kernels): al = squared column norm of G = (W + sigma I) V
        >= (0.5 |W|_F)^2 > 0.  W = 0 is not an iterate (W0 = e9 e9^T); a NaN iterate gives sigma = 1e-300 on the device (sqrt_fast(NaN)
        = 0) and NaN on the host, NaN columns in both; the certificate attempt sees them (the comment at fp_res in solve_quad_kernel says so).
      rcp(hn), rcp(wn), rcp(1 + ss) (the SO(3) Newton polish of both kernels): hn >= 1e-300 by its own guard (1 / hn overflows for
        hn < 2^-1022 in both builds alike: inf, then `lim` caps the step); wn > 0.5 is tested first; 1 + ss >= 1.
      rcp(g2) (the eigen-gradient step of the wave kernel): `g2 > 1e-6` is tested first.  rcp(n2), rsqrt_(n2), sqrt_fast(rad) (the twin candidates of the wave kernel): n2 = ta^2 + tb^2, the last
        entries of the top two unit eigenvectors, reached only when two eigenvalues dominate; zero only if both entries are exactly zero
        (Z99 = 1 keeps the top eigenspace off that); rad > 0 is tested first.
      rsqrt_(n2 > 1e-300 ? n2 : 1e-300) (inverse iteration, wave_kernel.h), rsqrt_(d > 0 ? d : 1) (ipm_wave.h, both uses), rcp_(d > 0 ? d : 1) (ipm_quad.h): guarded.
      fast_rcp(d) in the LDL^T pivots: the two of wave_kernel.h break at `!(d > 0)` first; cvxq::quad_ldl does not, a zero or NaN pivot breeds
        NaN below it, but minp <= 0 (or the earlier pivot that bred the NaN) is already recorded and the dual is rejected.
      rsqrt_(|n|^2) of a line's normal (assemble_kernel.h and the assembly phases of the quad and wave kernels; gram_add_line on the host): zero when the two image
        end points coincide.  Device NaN, host inf, and n = 0 * inf = NaN on the host as well: T, Q non-finite, ST_NONFINITE in both.
      sqrt_fast(fro) for sigma, sqrt_fast(r2) for fp_res (both kernels): a NaN sum gives 0, an inf sum NaN; discussed
        at fp_res in solve_quad_kernel -- the certificate attempt and the hand-over see the NaN iterate.
    No reachable argument makes the two builds disagree in status or pose: every special value either is excluded by a guard in front of
    the call, or makes the result non-finite in both builds, which the callers' own checks (written with `!(x > y)`) reject."""
    import hostsim

    bad = []
    for name, unit in SCALARS:
        y = dev.scalar(name, cases.SPECIALS, unit)
        got = [cases.classify(name, x, v) for x, v in zip(cases.SPECIALS, y)]
        host = hostsim.scalar("rcp" if name == "fast_rcp" else name, cases.SPECIALS)  # (fast_rcp has no host branch: beside rcp's)
        print(f"\n{name} [{unit}]")
        for x, v, g, h in zip(cases.SPECIALS, y, got, host):
            print(f"    x = {x!r:>24}  device {v!r:>24} ({g})   host {h!r}")
        if got != cases.special_row(name, unit):
            bad.append((name, unit, got))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------
# rotation parameters

ROTATIONS = [(n, u) for n in ("jacobi_cs", "jacobi_cs_dl", "jacobi_cs_dl_exact", "jacobi_cs_f32") for u in UNITS] + [("pair_cs", "c3"), ("pair_cs_f64", "c3")]
MARGIN = 4.0  # over the emulation's worst value on the same arguments: FMA contraction, seeds that are off by more than the model's one ulp


@pytest.fixture(scope="module")
def triples():
    return cases.rotation_arguments()


def run_rotation(dev, name, unit, al, be, gam):
    """device and emulation on the same arguments -> (device metrics, emulation metrics, device outputs, rot)"""
    a, rot, tie, d, apb = cases.rotation_case(name, al, be, gam)
    out = dev.rotation(name, cases.stack(a), rot, tie, unit)
    c, s, u = out[:, 0], out[:, 1], out[:, 2]
    assert np.isfinite(out).all()
    g = np.asarray(a[-1])
    md = cases.rotation_metrics(name, d[rot], g[rot], apb[rot], c[rot], s[rot], u[rot])
    ce, se, ue = cases.emulate(name, a, rot, tie, unit)
    me = cases.rotation_metrics(name, d[rot], g[rot], apb[rot], ce[rot], se[rot], ue[rot])
    return md, me, out, rot, a


@pytest.mark.parametrize("name,unit", ROTATIONS)
def test_rotation_parameters(dev, triples, name, unit):
    """Each of the six rotation forms on 2 M fixed-seed triples of the callers' domain (device_arithmetic_cases.rotation_arguments),
    rot computed as the caller computes it.  In long double, from what the function returned: (a) |c^2 + s^2 - 1|, (b) the inner
    product left after the rotation relative to |gam|, (c) the returned norm update (-t gam, or dl) against the change of |g_p|^2
    under the rotation actually applied, relative to al + be, (d) how far outside the inner rotation, max(0, |s| - c) -- each at most
    4x the worst value of the branch's numpy emulation on the same arguments."""
    md, me, out, rot, a = run_rotation(dev, name, unit, *triples)
    assert rot.all()
    print(f"\n{name} [{unit}]: " + "  ".join(f"{k} {md[k]:.3g} (emulation {me[k]:.3g})" for k in md))
    for k in md:
        assert md[k] <= MARGIN * me[k], (k, md[k], me[k])


@pytest.mark.parametrize("name,unit", ROTATIONS)
def test_rotation_parameters_at_the_edge_of_the_callers_domain(dev, name, unit):
    """be == al exactly and gam just past the callers' predicate, over the whole range of scales: where the 1e-37 guard of the
    single-precision forms weighs most (tests/test_device_arithmetic.py: test_the_guarded_half_angle_is_a_rotation_on_the_callers_domain).
    The same four figures within 4x the emulation's; for the guarded half-angle forms also the bound worked out there, row by row."""
    al, be, gam = cases.boundary_arguments()
    md, me, out, rot, a = run_rotation(dev, name, unit, al, be, gam)
    assert rot.sum() > 0.6 * len(rot)
    print(f"\n{name} [{unit}] at d = 0, gam^2 ~ 1e-30 al be: " + "  ".join(f"{k} {md[k]:.3g} (emulation {me[k]:.3g})" for k in md))
    for k in md:
        assert md[k] <= MARGIN * me[k], (k, md[k], me[k])
    if name in ("jacobi_cs_f32", "pair_cs"):
        unit_err = np.abs(out[:, 0].astype(cases.ld) ** 2 + out[:, 1].astype(cases.ld) ** 2 - 1).astype(np.float64)
        assert (unit_err[rot] <= cases.half_angle_bound(np.asarray(a[-1])[rot])).all()
    assert (out[~rot, 0] == 1).all() and (out[~rot, 1] == 0).all() and (out[~rot, 2] == 0).all()


@pytest.mark.parametrize("name,unit", ROTATIONS)
def test_no_rotation_is_the_identity_exactly(dev, name, unit):
    """(e) rot = false: c = 1, s = 0 and a zero update exactly, and no NaN anywhere -- on ordinary triples, on be == al, and on
    d = gam = 0 (where the exact forms' h2 is zero and the seed breeds a NaN that must be selected away)."""
    al, be, gam = cases.rotation_arguments(1001, seed=9)
    al = np.concatenate([al, [0, 0, 1, 1, 4, 0, 1e-300, 6.25e7]])
    be = np.concatenate([be, [0, 0, 1, 4, 1, 2, 1e-300, 6.25e7]])
    gam = np.concatenate([gam * 1e-17, [0, -0.0, 0, 0, 0, 0, 0, 1e-9]])
    a, rot, tie, d, apb = cases.rotation_case(name, al, be, gam)
    assert not rot.any()
    out = dev.rotation(name, cases.stack(a), rot, tie, unit)
    assert np.isfinite(out).all()
    assert (out[:, 0] == 1).all() and (out[:, 1] == 0).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("name", ["pair_cs", "pair_cs_f64"])
def test_the_two_lanes_of_a_pair_agree(dev, name):
    """(f) The quad kernel computes a pair's rotation twice, once in each lane: lane p sees (d, gam, tie 0), its partner (-d, gam, tie 1).
    The two must return the same c bit for bit and opposite s (else the two columns are rotated by different angles) -- including
    d = 0 and d = -0.0, where only the tie bit tells them apart."""
    al, be, gam = cases.rotation_arguments(100_003, seed=13)
    a, rot, tie, d, apb = cases.rotation_case(name, al, be, gam)
    d, g = a
    d = np.concatenate([d, np.zeros(64, d.dtype), -np.zeros(64, d.dtype)])
    g = np.concatenate([g, g[:128]])
    rot = np.ones(len(d), bool)
    p = dev.rotation(name, cases.stack((d, g)), rot, np.zeros(len(d), bool))
    q = dev.rotation(name, cases.stack((-d, g)), rot, np.ones(len(d), bool))
    assert (d == 0).sum() >= 128 and np.isfinite(p).all() and np.isfinite(q).all()
    assert (p[:, 0] == q[:, 0]).all() and (p[:, 0] > 0).all()  # (positive and finite: == is equality of the bits)
    assert (p[:, 1] == -q[:, 1]).all() and (p[:, 1] != 0).all()
    # and in the order the kernel has them when d = 0 the other way round: (d, tie 1) / (-d, tie 0)
    p = dev.rotation(name, cases.stack((d, g)), rot, np.ones(len(d), bool))
    q = dev.rotation(name, cases.stack((-d, g)), rot, np.zeros(len(d), bool))
    assert (p[:, 0] == q[:, 0]).all() and (p[:, 1] == -q[:, 1]).all() and (p[:, 1] != 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# eigen-solves


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("mode", ["f64", "exact"])
def test_psd_projection_matches_numpy_on_the_device(dev, unit, mode):
    """test_psd_projection_matches_numpy's body and bounds (tests/test_device_algorithm_hostsim.py) on the device build of cvx::Eig, with
    the single-precision rotation angles (exact off) and the float64 ones (exact on), plus the spectra the solver meets; then 1 031
    random symmetric matrices in one launch (more than one block, no multiple of 64).  Sweeps: at most 2 more than the host build
    on the same matrix (a rotation that leaves 4e-7 of the inner product standing costs at most that on the way to tol2 = 1e-30).

    What this test found (mode f64, both units, MI355X, ROCm 7.2.0): with cos(theta) refined by one plain Newton step from its float seed,
    the worst error / bound was 8.3 for Wp and 9.9 for the eigenvalues (1.2e-12 absolute) on the 1 031 matrices.  That step always
    undershoots (|c^2 + s^2 - 1| up to 1.8e-14, test_rotation_parameters), so every rotation shrank its two columns and the column norms
    -- the eigenvalues sqrt(n2) - sigma, and Wp with them -- came out low by a few 1e-14 of sigma after the ~40 rotations a column sees.
    jacobi_cs(double) now takes a third-order step (one FMA more); the figures with it are in DESIGN.md section 4."""
    import hostsim

    be = dev.backend(unit, mode)
    rs = np.random.RandomState(31)
    N = rs.normal(size=(1031 - 44, 10, 10))
    Ms = np.concatenate([np.array(cases.psd_projection_matrices() + cases.solver_spectra()), N + N.transpose(0, 2, 1)])
    W = np.array([cases.pack55(M) for M in Ms])
    Wp, lam, sw = be.pospart_batch(W)
    w, v = np.linalg.eigh(Ms)
    Mp = (v * np.maximum(w, 0)[:, None, :]) @ v.transpose(0, 2, 1)
    tol = 2e-14 * np.maximum(1.0, np.abs(w).max(1))
    eW = np.abs(np.array([cases.unpack55(x) for x in Wp]) - Mp).max(axis=(1, 2))
    eL = np.abs(np.sort(lam, axis=1) - w).max(1)
    _, _, sh = hostsim.pospart_batch(W)
    print(f"\nEig [{unit}, {mode}]: worst error / bound: Wp {(eW / tol).max():.3g}, eigenvalues {(eL / tol).max():.3g} (absolute {eL.max():.3g}); "
          f"sweeps device - host: max {(sw - sh).max()}, device max {sw.max()}")
    assert (sw <= sh + 2).all()
    assert (eW <= tol).all()
    assert (eL <= tol).all()
    cases.check_psd_projection_matches_numpy(be)
    cases.check_psd_projection_matches_numpy(be, cases.solver_spectra())


@pytest.mark.parametrize("unit", UNITS)
def test_single_precision_eigen_solve_on_the_device(dev, unit):
    """cvx::EigF (packed f2 columns, the half-angle rotation, the stopping test through v_rcp_f32): device and host instantiation each
    against numpy.linalg.eigh, relative to |W|_F; the device error is at most 4x the host's worst on the same matrices."""
    import hostsim

    Ms = cases.psd_projection_matrices() + cases.solver_spectra()
    W = np.array([cases.pack55(M) for M in Ms])
    res = {}
    for label, (Wp, lam, sw) in (("host", hostsim.pospart_batch(W, "f32")), ("device", dev.pospart_batch(W, "f32", unit))):
        worst = 0.0
        for M, wp, l in zip(Ms, Wp, lam):
            w, v = np.linalg.eigh(M)
            nrm = np.linalg.norm(M)
            worst = max(worst, np.abs(np.sort(l) - w).max() / nrm, np.abs(cases.unpack55(wp) - (v * np.maximum(w, 0)) @ v.T).max() / nrm)
        res[label] = (worst, sw)
    print(f"\nEigF [{unit}]: worst error / |W|_F: device {res['device'][0]:.3g}, host {res['host'][0]:.3g}; sweeps device max {res['device'][1].max()}, host max {res['host'][1].max()}")
    assert np.isfinite(res["device"][0]) and res["device"][0] <= 4 * res["host"][0]


# ------------------------------------------------------------------------------------------------------------------------------
# polar factors, projections, multipliers, assembly


@pytest.mark.parametrize("unit", UNITS)
def test_polar_factors(dev, unit):
    """polar3, near_rotation and inv3 on the device against numpy.linalg.svd's U Vh on 4 001 matrices in one launch: near-rotations as
    round_candidate passes them, reflections, condition numbers up to 1e6 -- the bounds of the host test
    (tests/test_device_arithmetic.py: test_polar_factor_host_build).  near_rotation is no polar factor (two polar steps, then
    Gram-Schmidt): its deviation from U Vh is held to 4x the host build's on the same inputs, its orthogonality to rounding.  An exactly
    singular matrix: rcp(det) is NaN on the device and inf on the host; both builds return a non-finite matrix, or both a finite one."""
    import hostsim

    be = dev.backend(unit)
    M, cond = cases.polar_inputs()
    ref = cases.polar_reference(M)
    eps = 2.0 ** -52
    R = be.polar3_batch(M, 40)
    err = np.abs(R - ref).max(axis=(1, 2))
    assert (err <= cases.POLAR_C * eps * cond).all()
    near = cond < 2
    R8 = be.polar3_batch(M[near], 8)
    assert (np.abs(R8 - ref[near]).max(axis=(1, 2)) <= cases.POLAR_C * eps * cond[near]).all()
    assert (np.sign(np.linalg.det(R)) == np.sign(np.linalg.det(M))).all()
    Mi, det = be.inv3_batch(M)
    assert (np.abs(det / np.linalg.det(M) - 1) <= cases.INV3_C * eps * cond ** 2).all()
    assert (np.abs(Mi @ M - np.eye(3)).max(axis=(1, 2)) <= cases.INV3_C * eps * cond ** 2).all()
    Rn, Rh = be.near_rotation_batch(M[near]), hostsim.near_rotation_batch(M[near])
    dn, dh = np.abs(Rn - ref[near]).max(), np.abs(Rh - ref[near]).max()
    print(f"\npolar [{unit}]: polar3 worst |R - U Vh| / (eps cond) {(err / (eps * cond)).max():.3g}; near_rotation |R - U Vh| device {dn:.3g}, host {dh:.3g}")
    assert dn <= 4 * dh
    assert np.abs(Rn.transpose(0, 2, 1) @ Rn - np.eye(3)).max() < 16 * eps
    # exactly singular: rank 2, rank 1, zero, a zero row
    S = np.array([np.diag([1.0, 1.0, 0.0]), np.outer([1.0, 2.0, 3.0], [1.0, 0.5, 0.25]), np.zeros((3, 3)), [[1, 2, 3], [0, 0, 0], [4, 5, 6.0]],
                  [[1, 2, 3], [2, 4, 6], [0, 1, 0.0]]])
    for f, g in ((be.polar3_batch, hostsim.polar3_batch), (be.near_rotation_batch, hostsim.near_rotation_batch)):
        with np.errstate(all="ignore"):
            fd, fh = np.isfinite(f(S)).all(axis=(1, 2)), np.isfinite(g(S)).all(axis=(1, 2))
        assert (fd == fh).all(), (fd, fh)


@pytest.mark.parametrize("unit", UNITS)
def test_affine_projection_matches_reference_constraints_on_the_device(dev, golden, unit):
    """the host test's body and bounds on the device build; the rc variant and a batch of 1 001 against the host build of the same
    closed form (1e-13, the bound the host test gives the form itself)"""
    import hostsim

    be = dev.backend(unit)
    cases.check_affine_projection_matches_reference_constraints(be, golden)
    X = np.random.RandomState(6).normal(size=(1001, 55))
    for homog in (False, True):
        for variant, host in ((0, hostsim.proj_affine), (1, hostsim.proj_affine_rc)):
            Y = dev.proj_affine_batch(X, homog, variant, unit)
            np.testing.assert_allclose(Y, np.array([host(x, homog) for x in X]), atol=1e-13)


@pytest.mark.parametrize("unit", UNITS)
def test_closed_form_dual_multipliers_match_reference_constraints_on_the_device(dev, golden, unit):
    cases.check_closed_form_dual_multipliers_match_reference_constraints(dev.backend(unit), golden)


@pytest.mark.parametrize("unit", UNITS)
def test_reuse_test_is_a_polar_factor_test_on_the_device(dev, unit):
    cases.check_reuse_test_is_a_polar_factor_test(dev.backend(unit))


@pytest.mark.parametrize("unit", UNITS)
def test_assembly_matches_reference_on_the_device(dev, golden, orc, unit):
    """test_assembly_matches_reference_g3, test_assembly_far_from_the_world_origin (its assembly half) and
    test_gram_sums_are_taken_about_a_robust_centre on cvx::assemble as the device pass compiles it (contracted Gram sums, rcp in inv3,
    rsqrt_ of the line normals): same references, same bounds."""
    be = dev.backend(unit)
    cases.check_assembly_matches_reference_g3(be, golden)
    cases.check_assembly_far_from_the_world_origin(be, orc, cases.far_origin_problem())
    cases.check_gram_sums_are_taken_about_a_robust_centre(be)
