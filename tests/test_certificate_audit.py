"""The certificate, checked from outside (CPU part).

DESIGN.md section 1.3 claims that status CERTIFIED proves the pose to be the global optimum of the relaxation:
0 <= cost - dobj <= eps.  Every other test reads both numbers from the code under test.  Here they are held against an independent
bracket  L <= p* <= U  of the SDP optimum in reference units (tests/certificate_audit.py: the oracle's multipliers made a rigorous
bound with numpy's eigvalsh on the reference's own constraint rows; the oracle's pose evaluated in long double):

  A0  R is a rotation, t = -B r
  A1  |cost - ||A r||^2_longdouble| <= k u tr A^T A          the reported cost is the reference's cost
  A2  dobj <= min(U, ||A r||^2) + k u tr A^T A               a lower bound cannot exceed a primal-feasible value
  A3  ||A r||^2 - L <= eps + k u tr A^T A                    eps-optimal by independent arithmetic (bracket width <= eps / 10)
  A4  certified twins (RANK_GT1 with a finite dobj): A0-A3, and the recovered poses have equal cost to eps

k = 32 x the float64 floor of the same quantity in the reference's own arithmetic (certificate_audit.FLOOR).  This file: the
bracket itself on fixed inputs, the audit's teeth, and the host build of the device algorithm (tests/hostsim).  The device:
test_certificate_audit_gpu.py.  Measured on 16 threads: this file takes 86 s, nearly all of it the oracle's solves of the
six-correspondence and minimal cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import certificate_audit as au  # noqa: E402

HOST_CASES = [(10, 0, 0.0, 256), (10, 0, 2.0, 256), (5, 5, 1.0, 128), (0, 6, 1.0, 64), (6, 0, 1.0, 64), (4, 0, 1.0, 64)]


def _hs_solve(d, n_p, n_l, **kw):
    import hostsim

    return hostsim.solve_batch(d["pts_2d"] if n_p else None, d["pts_3d"] if n_p else None, d["line_2d"] if n_l else None,
                               d["line_3d"] if n_l else None, d["K"], opts=hostsim.default_opts(**kw), want_Z=True)


def test_bracket_widths_on_fixed_inputs(orc):
    """40 problems per case, seeds 200 + n_p, synth.make_pnp.  Measured widths U - L: N = 10 at 2 px worst 4.4e-13, noise-free
    5.1e-14, N = 6 at 1 px 4.2e-14, N = 4 at 1 px: 37 of the 39 one-pose problems below 1e-10, worst 1.1e-8.  Asserted within 10 x."""
    from cvxpnpl_amd import synth

    for n_p, sigma, worst in ((10, 2.0, 4.4e-13), (10, 0.0, 5.1e-14), (6, 1.0, 4.2e-14), (4, 1.0, 1.1e-8)):
        n = 40
        d = synth.make_pnp(40, n_p, sigma, seed=200 + n_p)
        br = au.case_brackets(("width", n_p, sigma), d, n_p, 0, range(n))
        w = np.array([br[i]["w"] for i in range(n)])
        one = np.array([br[i]["n_poses"] == 1 for i in range(n)])
        print(f"bracket N={n_p} sigma={sigma}: worst width {w[one].max():.2e}, min {w.min():.2e}, {int((w[one] < 1e-10).sum())} of {int(one.sum())} below 1e-10")
        assert w.min() > -1e-15                              # L <= U: the bracket is a bracket (rounding of -b^T y in float64)
        assert w[one].max() <= 10 * worst, (n_p, sigma, w[one].max())
        if n_p == 4:
            assert (w[one] < 1e-10).sum() >= 0.85 * one.sum()
    # the rows' facts were asserted on loading; the rc rows too
    assert au.equality_rows(False)[0].shape == (22, 55) and au.equality_rows(True)[0].shape == (16, 55)


def _oracle_triple(b):
    """the oracle's own (R, t, cost, dobj): its pose, ||A r||^2 in float64, and its multipliers' rigorous bound"""
    R = b["R_o"]
    return R, -b["B"] @ au.vec(R), float(au.cost_ld(b["A"], R)), b["L"]


def test_the_audit_rejects_what_it_must(orc):
    """Teeth.  Ten points at 10 px noise (cost ~1e-3 tr Q, so that relative errors of 1e-9 in it are above the float64 floor):
    the oracle's own triple passes; each falsification named in the audit's contract is caught by the assertion meant for it."""
    from cvxpnpl_amd import synth

    d = synth.make_pnp(8, 10, 10.0, seed=210)
    br = au.case_brackets(("teeth", 10, 10.0), d, 10, 0, range(8))
    k = au.k_of("near")

    def fails(b, R, t, cost, dobj, tag):
        with pytest.raises(au.AuditFailure, match=tag):
            au.audit_one(b, R, t, cost, dobj, k)

    for i in range(8):
        b = br[i]
        assert b["w"] <= 1e-11, b["w"]
        R, t, cost, dobj = _oracle_triple(b)
        a = au.audit_one(b, R, t, cost, dobj, k)
        assert a["judged"] and a["over"] <= 1e-15 and a["gap"] <= 1e-11  # (over: the rounding of L itself)
        assert au.audit_one(b, R, t, cost, cost - 0.5e-9, k)["judged"]      # what the product writes: sound, and passes
        fails(b, R, t, cost, dobj + 1e-10, "A2")                             # a bound 1e-10 too high
        fails(b, R, t, cost, cost + 1e-10, "A2")                             # ... e.g. the 4 delta left out
        w = 1e-4 * np.array([0.6, -0.48, 0.64])                              # R rotated by 1e-4 rad, cost recomputed honestly
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]]) / th
        R2 = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ R
        U_, _, Vt = np.linalg.svd(R2)
        R2 = U_ @ Vt
        c2 = float(au.cost_ld(b["A"], R2))
        fails(b, R2, -b["B"] @ au.vec(R2), c2, dobj, "A3")                  # ... with a valid bound: not eps-optimal
        fails(b, R2, -b["B"] @ au.vec(R2), c2, c2 - 0.5e-9, "A2")           # ... with the bound the product would claim: above U
        fails(b, R, t, cost * (1 + 1e-9), dobj, "A1")                        # a cost off by 1e-9 relative
        fails(b, R, t, cost / b["trQ"], dobj / b["trQ"], "A1")               # normalised units
        fails(b, R, t, cost, dobj * max(b["trQ"], 1 / b["trQ"]), "A2")       # the bound alone in the wrong units (too high)
        fails(b, R, t + 1e-6, cost, dobj, "A0")
        fails(b, -R, -t, cost, dobj, "A0")
    # A3 leaves out what it cannot judge, and says so; the cap is enforced
    wide = dict(br[0], w=1e-9, L=br[0]["L"] - 1e-9)
    R, t, cost, dobj = _oracle_triple(br[0])
    assert not au.audit_one(wide, R, t, cost, dobj - 1e-9, k)["judged"]
    r = {"R": R[None], "t": t[None], "cost": np.array([[cost, dobj - 1e-9]]), "status": np.zeros(1, int)}
    with pytest.raises(AssertionError, match="could not judge"):
        au.audit_batch({0: wide}, r, [0], k, max_left_out=0.0)
    au.audit_batch({0: wide}, r, [0], k, max_left_out=1.0)


def _floor_cases():
    yield from (("near", au.parity_case(*c), c[0], c[1], False, c) for c in HOST_CASES + [(20, 9, 1.0, 67)])
    yield "near", au.rc_case(), 10, 0, True, "rc"
    yield "planar", au.planar_case(True), 10, 0, False, "planar-general"
    yield "planar", au.planar_case(False), 10, 0, False, "planar-canonical"
    yield "far", au.far_case(), 10, 0, False, "far"
    yield "large", au.large_case(), 2000, 0, False, "large"


def test_cost_floor_constants_hold(orc):
    """certificate_audit.FLOOR is the measured float64 floor of the cost in the reference's arithmetic: re-measured here on every
    audited case; a constant may not be below its measurement nor more than twice above the worst of its class."""
    worst = {}
    for cls, d, n_p, n_l, rc, key in _floor_cases():
        n = min(au.n_audit(n_p, n_l), len(d["pts_3d"] if n_p else d["line_3d"]))
        f = au.measure_cost_floor(d, n_p, n_l, range(n), key, rc=rc, centred=(cls == "far"))
        print(f"cost floor {key}: {f:.3g} u tr Q  (class {cls})")
        if cls == "far":   # as the reference forms C and N, about the far origin: eight digits lost (recorded in certificate_audit.FLOOR)
            fu = au.measure_cost_floor(d, n_p, n_l, range(n), key, rc=rc)
            print(f"cost floor {key}, uncentred: {fu:.3g} u tr Q")
            assert 1e7 < fu < 1e9
        worst[cls] = max(worst.get(cls, 0.0), f)
    for cls, f in worst.items():
        assert f <= au.FLOOR[cls] <= 2.0 * f, (cls, f, au.FLOOR[cls])


@pytest.mark.parametrize("opts", [{}, {"dual_shift": 0.0}, {"dual_refine": 0}], ids=["default", "no-shift", "no-refine"])
@pytest.mark.parametrize("n_p,n_l,sigma,batch", HOST_CASES)
def test_host_build_certificates(orc, n_p, n_l, sigma, batch, opts):
    """every certified problem among the first 64 (24 for N = 4) of a case, host build of the device algorithm"""
    d = au.parity_case(n_p, n_l, sigma, batch)
    n = au.n_audit(n_p, n_l)
    br = au.case_brackets((n_p, n_l, sigma, batch), d, n_p, n_l, range(n))
    r = _hs_solve(d, n_p, n_l, **opts)
    idx = np.flatnonzero(au.certified(r)[:n])
    assert len(idx) >= (0.5 * n if n_p + n_l <= 4 else n - 1)
    au.audit_batch(br, r, idx, au.k_of("near"), max_left_out=0.15 if n_p + n_l <= 4 else 0.0, label=f"hostsim {n_p}/{n_l} s={sigma} {opts}")


@pytest.mark.parametrize("general", [False, True], ids=["canonical", "general"])
def test_host_build_planar_twins(orc, general):
    """A4: planar scenes leave as RANK_GT1 with a certificate for the pair; both recovered poses cost the same to eps"""
    import cvxpnpl_amd as ca

    d = au.planar_case(general)
    br = au.case_brackets("planar-general" if general else "planar-canonical", d, 10, 0, range(64))
    r = _hs_solve(d, 10, 0)
    idx = np.flatnonzero(au.certified(r))
    assert len(idx) >= 60 and (r["status"][idx] == 1).all(), np.bincount(r["status"])
    au.audit_batch(br, r, idx, au.k_of("planar"), label=f"hostsim planar general={general}")
    _audit_twins(ca, br, r, idx)


def _audit_twins(ca, br, r, idx, min_pairs=0.9):
    n2 = 0
    for i in idx:
        b = br[int(i)]
        poses = ca.recover_multi(r["Z"][i], b["B"].reshape(27))
        if len(poses) != 2:
            continue
        c = [au.cost_ld(b["A"], R) for R, _ in poses]
        assert abs(float(c[0] - c[1])) <= au.EPS, (i, float(c[0]), float(c[1]))
        assert min(abs(float(ci - au.cost_ld(b["A"], r["R"][i]))) for ci in c) <= au.EPS      # the returned pose is one of them
        n2 += 1
    assert n2 >= min_pairs * len(idx), (n2, len(idx))


def test_host_build_far_origin(orc):
    d = au.far_case()
    br = au.case_brackets("far", d, 10, 0, range(64))
    r = _hs_solve(d, 10, 0)
    idx = np.flatnonzero(au.certified(r))
    assert len(idx) >= 63
    au.audit_batch(br, r, idx, au.k_of("far"), label="hostsim far origin")


def test_host_build_rc_variant(orc):
    """the 16-row constraint set through the cost seam, with the test's own A^T A and B"""
    import hostsim

    d = au.rc_case()
    br = au.case_brackets("rc", d, 10, 0, range(64), rc=True)
    Q45 = np.array([au.pack_upper(br[i]["A"].T @ br[i]["A"]) for i in range(64)])
    B27 = np.array([br[i]["B"].reshape(27) for i in range(64)])
    r = hostsim.solve_cost_batch(Q45, B27, variant=1, want_Z=True)
    idx = np.flatnonzero(au.certified(r))
    assert len(idx) >= 60, np.bincount(r["status"])
    au.audit_batch(br, r, idx, au.k_of("near"), max_left_out=0.15, label="hostsim rc")
    # the full set at the same seam
    brf = au.case_brackets("rc-inputs-full", d, 10, 0, range(64))
    rf = hostsim.solve_cost_batch(Q45, B27, variant=0, want_Z=True)
    idx = np.flatnonzero(au.certified(rf))
    assert len(idx) >= 63
    au.audit_batch(brf, rf, idx, au.k_of("near"), label="hostsim cost seam")


@pytest.mark.parametrize("option,batch", [("dual_shift", 4000), ("dual_refine", 6000)])
def test_host_build_rescued_certificates(orc, option, batch):
    """The certificates the second tries (S1 + m D(R)) and the eigen-gradient step (S1 + tau P_U(n n^T)) hand out: problems
    certified in fewer iterations with the option on than off (the selection of test_dual_retry.py), at most 128 of them."""
    from cvxpnpl_amd import synth

    d = synth.make_pnpl(batch, 10, 0, 2.0, seed=42)
    off = _hs_solve(d, 10, 0, **{option: 0.0 if option == "dual_shift" else 0})
    on = _hs_solve(d, 10, 0)
    resc = np.flatnonzero((on["status"] == 0) & (on["iters"] < off["iters"]))[:128]
    assert len(resc) >= 10, len(resc)
    br = au.case_brackets(("rescued", batch), d, 10, 0, resc)
    au.audit_batch(br, on, resc, au.k_of("near"), label=f"hostsim rescued by {option}")
