"""pose_step, damped_step and step_measure of csrc/refine_core.h on their own (tests/hostsim/refine_shim.cpp, built with g++), against
long-double restatements.  The refinement tests only ever see them through a converged pose, where a step is below 0.05 rad and the
damping is where the schedule left it.  No GPU needed."""
import numpy as np
import pytest

import refine_cases as rc
import refine_reference as ref

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def _rodrigues_ld(w):
    """exp([w]x) in long double: I + sin(th) / th W + 2 sin(th / 2)^2 / th^2 W^2 (the second form has no cancellation at small th)."""
    w = np.asarray(w, LD)
    th = np.sqrt(w @ w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)
    if th == 0:
        return np.eye(3, dtype=LD)
    a = np.sin(th) / th
    s = np.sin(th / 2) / th
    return np.eye(3, dtype=LD) + a * W + 2 * s * s * (W @ W)


@pytest.mark.parametrize("th", [0.0, 1e-160, 1e-12, 1e-6, 1e-2, 1.0, np.pi, 6.0, 8.0, 20.0])
def test_pose_step_is_the_exponential_map(th):
    """R^T R - I <= 16 eps whatever |w| is; the rotation itself to 16 eps for |w| <= 8 (beyond, the header claims a rotation, not this
    one: the Taylor polynomials are truncated for a half angle over 32 of at most 1/8); the translation part is one addition, exact."""
    import hostsim

    rs = np.random.RandomState(int(th * 1000) % 1000 + 3)
    worst_orth = worst_err = 0.0
    for _ in range(20):
        ax = rs.normal(size=3)
        ax /= np.linalg.norm(ax)
        tau, tc = rs.normal(size=3), rs.normal(size=3)
        d = np.concatenate([th * ax, tau])
        E, t1 = hostsim.pose_step(np.eye(3), tc, d)
        assert np.isfinite(E).all()
        assert t1.tobytes() == (tc + tau).tobytes()
        worst_orth = max(worst_orth, float(np.abs(E.astype(LD).T @ E.astype(LD) - np.eye(3)).max()))
        worst_err = max(worst_err, float(np.abs(E.astype(LD) - _rodrigues_ld(d[:3])).max()))
        # ... and it multiplies R from the left: against the long-double product with a rotation that is not the identity
        R = ref.expm_so3(rs.normal(size=3))
        R1, _ = hostsim.pose_step(R, tc, d)
        worst_orth = max(worst_orth, float(np.abs(R1.astype(LD).T @ R1.astype(LD) - R.astype(LD).T @ R.astype(LD)).max()))
        if th <= 8.0:
            worst_err = max(worst_err, float(np.abs(R1.astype(LD) - _rodrigues_ld(d[:3]) @ R.astype(LD)).max()))
    print(f"|w| = {th:g}: orthonormality {worst_orth / EPS:.2f} eps, rotation error {worst_err / EPS:.2f} eps")
    assert worst_orth <= 16 * EPS
    if th <= 8.0:
        assert worst_err <= 16 * EPS


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in long double (numpy's solve has no long-double path)."""
    A, b = np.array(A, LD), np.array(b, LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            b[i] -= f * b[k]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


@pytest.fixture(scope="module")
def normal_equations():
    """J^T J and J^T r of problem 0 of the six shapes at its start, from the reference's Jacobian."""
    out = {}
    for n_p, n_l, sigma in rc.SHAPES:
        d, R0, t0, kw = rc.problem(1, n_p, n_l, sigma)
        data = rc.one(kw, 0)
        J = ref.jacobian(d["K"], R0[0], t0[0], **data)
        r, _ = ref.residuals(d["K"], R0[0], t0[0], **data)
        out[(n_p, n_l)] = (J.T @ J, J.T @ r)
    return out


@pytest.mark.parametrize("lam", [1e-12, 1e-3, 1e6])
@pytest.mark.parametrize("shape", [s[:2] for s in rc.SHAPES])
def test_damped_step_solves_the_damped_system(normal_equations, shape, lam):
    import hostsim

    A, g = normal_equations[shape]
    M = A + lam * np.diag(np.diag(A))
    want = _solve_ld(M.astype(LD) , -g.astype(LD))
    # (the damped matrix in long double: A_ii (1 + lam) is rounded once by the library too, and that rounding is inside cond eps)
    ok, d = hostsim.damped_step(A, g, lam)
    err = float(np.linalg.norm(d.astype(LD) - want) / np.linalg.norm(want))
    bound = 1e2 * np.linalg.cond(M) * EPS
    print(f"{shape} lambda={lam:g}: cond {np.linalg.cond(M):.1e}, relative error {err:.1e}, bound {bound:.1e}")
    assert ok and err <= bound


def test_damped_step_refuses_what_it_cannot_factor(normal_equations):
    import hostsim

    A, g = normal_equations[(10, 0)]
    Z = A.copy()
    Z[2, :] = 0.0
    Z[:, 2] = 0.0                                                # a zero diagonal entry: no damping lifts it
    for lam in (1e-3, 1e6):
        ok, d = hostsim.damped_step(Z, g, lam)
        assert not ok and d.tobytes() == np.zeros(6).tobytes()
    for i, j in ((0, 0), (1, 4), (5, 5)):
        N = A.copy()
        N[i, j] = N[j, i] = np.nan
        ok, d = hostsim.damped_step(N, g, 1e-3)
        assert not ok and d.tobytes() == np.zeros(6).tobytes(), (i, j)
    gn = g.copy()
    gn[3] = np.nan
    ok, d = hostsim.damped_step(A, gn, 1e-3)
    assert not ok and d.tobytes() == np.zeros(6).tobytes()


def test_step_measure_is_the_public_chart_norm():
    """|(w, tau_c + (R c) x w)| / (1 + |t|), t = tc - R c, against long double."""
    import hostsim

    rs = np.random.RandomState(9)
    for scale in (1.0, 1e3, 1e6):
        R = ref.expm_so3(rs.normal(size=3))
        c, tc, d = scale * rs.normal(size=3), rs.normal(size=3), 1e-3 * rs.normal(size=6)
        Rc = R.astype(LD) @ c.astype(LD)
        tau = d[3:].astype(LD) + np.cross(Rc, d[:3].astype(LD))
        want = np.sqrt(d[:3].astype(LD) @ d[:3].astype(LD) + tau @ tau) / (1 + np.sqrt((tc - Rc) @ (tc - Rc)))
        got = hostsim.step_measure(R, tc, c, d)
        assert abs(got - want) <= 16 * EPS * want, (scale, got, want)
