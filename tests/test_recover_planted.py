"""The host build of the rank > 1 recovery (csrc/recover_core.h through cvxpnpl_recover_multi[_batch]) against planted
multi-pose solutions: Z = sum_i w_i z_i z_i^T with known rotations, so the exact answer is known (tests/recover_reference.py,
tests/golden/recover_planted.npz).  No GPU, no solve.

The rules (recover_reference.judge):
  * pose counts follow the numpy rank rule (eigvalsh at 1e-3) on the k = 2 / 4 / rank-1 classes and both threshold members;
  * unpolished k = 2 / 4: per problem err <= 10 x the reference's own error + 1e-12, the same for t scaled by
    max(1, |B|_inf); the floor alone where the reference returns NaN (planar twins); a k = 4 problem on which the reference
    is worse than 1e-6 is held to 1e-6, and at most 10 % of a class may be such problems;
  * polished (a cost whose null space holds the planted rotations, Hessian condition <= 1e3): 2.5e-11 = 100 x 1e3 x u,
    with and without 1e-8 noise on Z -- the polish is a Newton solve on Q, not on Z;
  * slots beyond n_poses are NaN, whatever the caller put there.
"""
import ctypes as C

import numpy as np
import pytest
import recover_reference as rr

SENTINEL = 7.25
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def L():
    from cvxpnpl_amd import _lib, build

    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return rr.load_fixture()


def _dp(a):
    return a.ctypes.data_as(DP) if a is not None else None


def single(L, Z55, B27, Q45=None):
    """cvxpnpl_recover_multi through the raw C ABI, outputs pre-filled with a sentinel: (n, R [4,3,3], t [4,3])."""
    Z55, B27 = np.ascontiguousarray(Z55, dtype=np.float64), np.ascontiguousarray(B27, dtype=np.float64)
    Q45 = np.ascontiguousarray(Q45, dtype=np.float64) if Q45 is not None else None
    R, t = np.full((4, 3, 3), SENTINEL), np.full((4, 3), SENTINEL)
    n = L.cvxpnpl_recover_multi(_dp(Z55), _dp(B27), _dp(Q45), _dp(R), _dp(t))
    return n, R, t


def batch(L, status, Z, B, Q, n_threads):
    """cvxpnpl_recover_multi_batch through the raw C ABI, outputs pre-filled with a sentinel."""
    n = len(Z)
    Z, B = np.ascontiguousarray(Z, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    Q = np.ascontiguousarray(Q, dtype=np.float64) if Q is not None else None
    st = np.ascontiguousarray(status, dtype=np.int32) if status is not None else None
    R, t, cnt = np.full((n, 4, 3, 3), SENTINEL), np.full((n, 4, 3), SENTINEL), np.full(n, -99, dtype=np.int32)
    rc = L.cvxpnpl_recover_multi_batch(n, st.ctypes.data_as(IP) if st is not None else None, _dp(Z), _dp(B), _dp(Q), _dp(R), _dp(t),
                                       cnt.ctypes.data_as(IP), n_threads)
    assert rc == 0
    return cnt, R, t


def run_class(L, cls, with_q):
    out = [single(L, cls["Z55"][i], cls["B27"][i], cls["Q45"][i] if with_q else None) for i in range(len(cls["Z55"]))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def test_fixture_is_what_the_rules_assume(fx):
    """From numpy alone: every eigenvalue clear of the rank threshold, the intended ranks, the polish costs' null space and
    conditioning, the share of k = 4 problems on which the reference is worse than 1e-6, and the reference's recorded error
    recomputed from its recorded poses."""
    for name, (k, n) in rr.CLASSES.items():
        cls = fx[name]
        assert cls["Z55"].shape == (n, 55) and cls["R"].shape == (n, k, 3, 3) and cls["B27"].shape == (n, 27), name
        want_rank = 1 if name == "thr_lo" else k
        for i in range(n):
            assert rr.rank_margin(cls["Z55"][i]) >= rr.RANK_MARGIN, (name, i)
            assert rr.np_rank(cls["Z55"][i]) == want_rank, (name, i)
            m = cls["ref_n"][i]
            if np.isfinite(cls["ref_R"][i, :m]).all():
                assert rr.rot_err(cls["ref_R"][i, :m], cls["R"][i])[0] == cls["ref_err"][i], (name, i)
            else:
                assert np.isnan(cls["ref_err"][i]), (name, i)
    lam2 = {name: np.array([rr.eigenvalues(z)[-2] for z in fx[name]["Z55"]]) for name in rr.THRESHOLD}
    assert np.allclose(lam2["thr_hi"], 2e-3, rtol=1e-6) and np.allclose(lam2["thr_lo"], 5e-4, rtol=1e-6)
    for name in rr.POLISHED:
        cls = fx[name]
        for i in range(len(cls["Z55"])):
            Q = rr.unpack_q45(cls["Q45"][i])
            for R in cls["R"][i]:
                assert np.abs(Q @ rr.vec(R)).max() <= 1e-13 * np.trace(Q), (name, i)
            assert rr.hessian_cond(Q, cls["R"][i]) <= rr.KAPPA_MAX, (name, i)
    for name in rr.UNPOLISHED_K4:
        assert (fx[name]["ref_err"] > rr.DESIGN_BOUND).mean() <= 0.10, name
    for name in rr.UNPOLISHED_K2:  # no k = 2 problem is left out of the rule: the reference is finite or NaN, never merely bad
        e = fx[name]["ref_err"]
        assert (np.isnan(e) | (e < 1e-11)).all(), name
    assert np.isnan(fx["planar_eq"]["ref_err"]).sum() >= 16  # the case the planar classes are there for


@pytest.mark.parametrize("name", rr.UNPOLISHED_K2 + rr.UNPOLISHED_K4 + rr.RANK1 + rr.THRESHOLD)
def test_unpolished_recovery_returns_the_planted_poses(L, fx, name):
    cls = fx[name]
    cnt, R, t = run_class(L, cls, with_q=False)
    res = rr.judge(name, cls, cnt, R, t)
    print(rr.figures(name, res, cls))
    if name.startswith("planar"):
        assert (cnt == 2).all() and np.isfinite(R[:, :2]).all() and np.isfinite(t[:, :2]).all()


@pytest.mark.parametrize("name", rr.POLISHED)
def test_polished_recovery_returns_the_planted_poses(L, fx, name):
    cls = fx[name]
    cnt, R, t = run_class(L, cls, with_q=True)
    res = rr.judge(name, cls, cnt, R, t)
    print(rr.figures(name, res, cls))


def test_reflection_is_left_unpolished_and_finite(L, fx):
    """A candidate with det R < 0 (a rank-1 Z planted from an improper orthogonal matrix) is not polished: with a generic cost
    that is no null-space cost it comes back finite and bit for bit as without a cost.  The same cost does move a proper
    candidate, so the polish was live."""
    rs = np.random.RandomState(5)
    M = rs.normal(size=(9, 12))
    q45 = rr.pack_q45(M @ M.T)
    B27 = fx["r1_exact"]["B27"][0]
    proper = fx["r1_exact"]["R"][0, 0]
    improper = proper @ np.diag([1.0, 1.0, -1.0])
    n0, R0, t0 = single(L, rr.vech10(rr.plant_Z([improper], [1.0])), B27)
    n1, R1, t1 = single(L, rr.vech10(rr.plant_Z([improper], [1.0])), B27, q45)
    assert n0 == n1 == 1 and np.linalg.det(R0[0]) < 0
    assert np.isfinite(R1[0]).all() and np.isfinite(t1[0]).all()
    assert np.array_equal(R0, R1, equal_nan=True) and np.array_equal(t0, t1, equal_nan=True)
    assert np.abs(R0[0] - improper).max() < 1e-14
    n2, R2, _ = single(L, rr.vech10(rr.plant_Z([proper], [1.0])), B27, q45)
    assert n2 == 1 and np.isfinite(R2[0]).all() and np.abs(R2[0] - proper).max() > 1e-3
    assert np.abs(R2[0] @ R2[0].T - np.eye(3)).max() < 1e-14


@pytest.mark.parametrize("name", rr.ODD)
def test_odd_and_high_ranks_are_recorded(L, fx, name):
    """Rank 3 / 5 / 6: the basis is padded (rank 3) or cut (rank 5, 6) to four vectors as in the reference, and the planted poses
    are in general NOT among the four returned ones.  Counts are 2 or 4, every slot is a finite orthogonal
    matrix or NaN; how many planted poses are found is printed, not asserted."""
    cls = fx[name]
    cnt, R, t = run_class(L, cls, with_q=False)
    found = rr.check_odd(name, cls, cnt, R, t)
    ref_found = sum(int((np.sqrt(((cls["ref_R"][i][None, :cls["ref_n"][i]] - cls["R"][i][:, None]) ** 2).sum(axis=(2, 3))).min(axis=1) < 1e-6).sum())
                    for i in range(len(cnt)))
    print(f"{name}: {found} of {cls['R'].shape[0] * cls['R'].shape[1]} planted poses found (reference: {ref_found})")


def test_output_contract_single_call(L, fx):
    """Slots k >= max(n, 0) come back NaN whatever was there; NaN and all-zero Z give -1."""
    for name, want in (("k2_rand_w25", 2), ("k4_rand_w25", 4), ("r1_exact", 1), ("thr_lo", 1)):
        n, R, t = single(L, fx[name]["Z55"][0], fx[name]["B27"][0])
        assert n == want
        assert np.isfinite(R[:n]).all() and np.isfinite(t[:n]).all()
        assert np.isnan(R[n:]).all() and np.isnan(t[n:]).all()
    B27 = fx["k2_rand_w25"]["B27"][0]
    for Z55 in (np.full(55, np.nan), np.zeros(55), np.where(np.arange(55) == 17, np.nan, fx["k2_rand_w25"]["Z55"][0])):
        n, R, t = single(L, Z55, B27)
        assert n == -1 and np.isnan(R).all() and np.isnan(t).all()


def _mixed_batch(fx):
    """Every class in one batch, with the statuses 1 (flagged), 0, 2, 3, 4 (skipped) dealt round and a NaN Z every 7th."""
    names = tuple(rr.CLASSES)
    Z, B, Q, who = rr.concat(names, fx)
    Z = Z.copy()
    status = np.array([(1, 1, 0, 1, 2, 1, 3, 1, 4)[i % 9] for i in range(len(Z))], dtype=np.int32)
    Z[3::7] = np.nan
    return Z, B, Q, status


@pytest.mark.parametrize("n_threads", (1, 3, 16))
def test_batch_equals_single_calls_and_fills_skipped_slots(L, fx, n_threads):
    Z, B, Q, status = _mixed_batch(fx)
    for q in (None, Q):
        cnt, R, t = batch(L, status, Z, B, q, n_threads)
        for i in range(len(Z)):
            if status[i] != 1:
                assert cnt[i] == 0 and np.isnan(R[i]).all() and np.isnan(t[i]).all(), i
                continue
            n, R1, t1 = single(L, Z[i], B[i], q[i] if q is not None else None)
            assert cnt[i] == n, i
            assert np.array_equal(R[i], R1, equal_nan=True) and np.array_equal(t[i], t1, equal_nan=True), i
            if np.isnan(Z[i]).any():
                assert n == -1 and np.isnan(R[i]).all() and np.isnan(t[i]).all()
    # status == NULL: every problem is recovered
    cnt_all, R_all, t_all = batch(L, None, Z, B, None, n_threads)
    assert (cnt_all != 0).all() and not (R_all == SENTINEL).any() and not (t_all == SENTINEL).any()
    m = status == 1
    cnt1, R1, t1 = batch(L, status, Z, B, None, n_threads)
    assert np.array_equal(cnt_all[m], cnt1[m]) and np.array_equal(R_all[m], R1[m], equal_nan=True) and np.array_equal(t_all[m], t1[m], equal_nan=True)


def test_batch_bad_arguments(L, fx):
    Z, B, Q, status = _mixed_batch(fx)
    R, t, cnt = np.zeros((len(Z), 4, 3, 3)), np.zeros((len(Z), 4, 3)), np.zeros(len(Z), dtype=np.int32)
    ip = cnt.ctypes.data_as(IP)
    assert L.cvxpnpl_recover_multi_batch(0, None, _dp(Z), _dp(B), None, _dp(R), _dp(t), ip, 1) == 0
    assert L.cvxpnpl_recover_multi_batch(-1, None, _dp(Z), _dp(B), None, _dp(R), _dp(t), ip, 1) == -1
    assert L.cvxpnpl_recover_multi_batch(4, None, None, _dp(B), None, _dp(R), _dp(t), ip, 1) == -1
    assert L.cvxpnpl_recover_multi_batch(4, None, _dp(Z), _dp(B), None, None, _dp(t), ip, 1) == -1
    assert L.cvxpnpl_recover_multi_batch(4, None, _dp(Z), _dp(B), None, _dp(R), _dp(t), None, 1) == -1


# ------------------------------------------------------------------------------------------------- the root finder alone
def _quartics():
    """(name, real roots, or None with coefficients): clusters, a double root, magnitudes spread over eight decades, a lost
    leading coefficient, a complex pair.  The planted classes never get there: the rank threshold keeps their roots apart."""
    cases = []
    for d in (1e-2, 1e-4, 1e-6):
        cases.append((f"pair {d:g} apart", np.array([-1.5, 0.5, 1.0, 1.0 + d])))
        cases.append((f"pair {d:g} apart, large", np.array([-300.0, 200.0, 200.0 * (1 + d), 700.0])))
    cases.append(("three within 1e-3", np.array([2.0, 2.001, 2.002, -1.0])))
    cases.append(("spread 1e-4 .. 1e4", np.array([1e-4, -0.03, 7.0, 1e4])))
    cases.append(("spread 1e-3 .. 1e3", np.array([-1e-3, 1.0, 30.0, -1e3])))
    cases.append(("tiny and huge", np.array([1e-6, 2e-6, 1.0, 1e5])))
    rs = np.random.RandomState(11)
    for i in range(8):
        cases.append((f"random {i}", rs.normal(size=4) * 10.0 ** rs.uniform(-2, 2, size=4)))
    return cases


def _horner_abs(p, z):
    """(|p(z)|, sum |p_k| |z|^(n-k)) in extended precision."""
    p = np.asarray(p, dtype=np.longdouble)
    zr, zi = np.longdouble(z.real), np.longdouble(z.imag)
    fr, fi = np.longdouble(0), np.longdouble(0)
    az, mag = np.hypot(zr, zi), np.longdouble(0)
    for c in p:
        fr, fi = fr * zr - fi * zi + c, fr * zi + fi * zr
        mag = mag * az + abs(c)
    return float(np.hypot(fr, fi)), float(mag)


# A root rounded to the nearest double leaves |p(z)| <= u |z| |p'(z)| <= 4 u ptilde(|z|) for a quartic (ptilde: the polynomial of the
# absolute coefficients); the last Newton step is itself computed with a complex Horner evaluation whose error is at most
# 2 n sqrt(5) u ptilde = 18 u ptilde.  Together 22 u, taken as 32 u.
BACKWARD = 32 * rr.U


@pytest.mark.parametrize("name,roots", _quartics(), ids=[c[0] for c in _quartics()])
def test_root_finder_backward_error(name, roots):
    """cvxr::poly_roots on quartics with known real roots: four roots come back, every one with a residual at rounding level
    (it is the exact root of a polynomial whose coefficients differ by BACKWARD relative), and every simple, well-separated
    true root has a computed root within the first-order bound BACKWARD ptilde(|r|) / |p'(r)|, doubled for the higher orders."""
    import hostsim

    for lead in (1.0, -3.7e-5, 2.5e6):
        p = lead * np.poly(roots)
        z = hostsim.poly_roots(p)
        assert len(z) == 4 and np.isfinite(z).all(), (name, lead, z)
        for zi in z:
            res, mag = _horner_abs(p, zi)
            assert res <= BACKWARD * mag, (name, lead, zi, res / mag / rr.U)
        dp = np.polyder(p)
        used = set()
        for r in roots:
            sep = np.abs(np.delete(roots, np.argmin(np.abs(roots - r))) - r).min()
            fwd = 2 * BACKWARD * _horner_abs(p, complex(r))[1] / abs(np.polyval(dp, r))
            j = int(np.argmin(np.abs(z - r)))
            if fwd < 0.1 * sep:
                assert abs(z[j] - r) <= fwd + 4 * rr.U * abs(r), (name, lead, r, z[j], fwd)
                assert j not in used, (name, lead, "two true roots share one computed root")
                used.add(j)


def test_root_finder_degenerate_leading_coefficients():
    """Exact zeros in front: the degree drops and the remaining roots are found; an all-zero polynomial has none."""
    import hostsim

    z = hostsim.poly_roots([0.0, 2.0, -6.0, -8.0, 24.0])  # 2 (x - 3)(x - 2)(x + 2)
    assert len(z) == 3 and np.abs(np.sort(z.real) - np.array([-2.0, 2.0, 3.0])).max() < 1e-14 and np.abs(z.imag).max() < 1e-14
    z = hostsim.poly_roots([0.0, 0.0, 1.0, 0.0, -4.0])
    assert len(z) == 2 and np.abs(np.sort(z.real) - np.array([-2.0, 2.0])).max() < 1e-15
    assert len(hostsim.poly_roots([0.0, 0.0, 0.0, 0.0, 5.0])) == 0
    z = hostsim.poly_roots([1.0, 0.0, 3.0, 0.0, -4.0])  # (x^2 - 1)(x^2 + 4): a complex pair next to two real roots
    assert sorted(np.round(z.real, 12)) == [-1.0, 0.0, 0.0, 1.0] and sorted(np.round(z.imag, 12)) == [-2.0, 0.0, 0.0, 2.0]
