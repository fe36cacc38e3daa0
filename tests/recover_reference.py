"""Planted multi-pose solutions: an exact reference for the rank > 1 recovery (csrc/recover_core.h).

Take distinct rotations R_1..R_k, weights w_i > 0 and z_i = [vec(R_i); 1] (column-major vec).  Z = sum_i w_i z_i z_i^T has
rank k generically, and the rotations in its range that satisfy the 21 quadratic identities of a rotation matrix are exactly
the planted ones: the recovery must return the set {R_i} with t = -B vec(R_i), to rounding times the conditioning of the
root problem.  No solver is involved.

numpy only; nothing here imports the package under test.  tests/golden/make_golden_recover.py draws the committed fixture
(tests/golden/recover_planted.npz) with these generators and adds what the reference makes of every Z; the tests read the
fixture and use the metrics below.
"""
import functools
import os

import numpy as np

U = 2.0 ** -53                 # unit roundoff of float64
RANK_TOL = 1e-3                # cvxpnpl.py:502: rank = #(eigenvalues > 1e-3)
RANK_MARGIN = 1e-4             # no fixture eigenvalue lies this close to RANK_TOL
FLOOR = 1e-12                  # 4 500 u on entries of size one: the reference lands on 1e-16 by luck on some problems
FACTOR = 10.0                  # margin over the reference for a different but equivalent elimination
DESIGN_BOUND = 1e-6            # what a k = 4 problem is held to where the reference itself is worse
KAPPA_MAX = 1e3                # polish classes: Hessian condition number at every planted rotation
POLISH_BOUND = 2.5e-11         # 100 * KAPPA_MAX * u = 2.3e-11, rounded up
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recover_planted.npz")

_IU10 = np.triu_indices(10)
_IU9 = np.triu_indices(9)


# ---------------------------------------------------------------------------------------------------------- packing
def vech10(M):
    """Symmetric 10x10 -> 55 entries, the order of cvxpnpl.py:346-370 (columns of the lower triangle = rows of the upper)."""
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64)[_IU10])


def vech10_inv(v):
    M = np.zeros((10, 10))
    M[_IU10] = v
    return M + np.triu(M, 1).T


def pack_q45(Q):
    """Symmetric 9x9 cost -> the 45 entries the C ABI takes (rows of the upper triangle)."""
    return np.ascontiguousarray(np.asarray(Q, dtype=np.float64)[_IU9])


def unpack_q45(q):
    M = np.zeros((9, 9))
    M[_IU9] = q
    return M + np.triu(M, 1).T


def vec(R):
    """Column-major vec of a 3x3 (the r of t = -B r)."""
    return np.asarray(R, dtype=np.float64).T.reshape(9)


def z_of(R):
    return np.append(vec(R), 1.0)


# ------------------------------------------------------------------------------------------------------- generators
def rodrigues(aa):
    aa = np.asarray(aa, dtype=np.float64)
    ang = np.linalg.norm(aa)
    if ang == 0.0:
        return np.eye(3)
    k = aa / ang
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def rand_axis(rs):
    a = rs.normal(size=3)
    return a / np.linalg.norm(a)


def rand_rotation(rs):
    """Uniform on SO(3) (QR of a Gaussian matrix, signs fixed)."""
    Qm, Rm = np.linalg.qr(rs.normal(size=(3, 3)))
    Qm = Qm * np.sign(np.diag(Rm))
    if np.linalg.det(Qm) < 0:
        Qm[:, 2] = -Qm[:, 2]
    return Qm


def rotations_random(rs, k):
    return np.stack([rand_rotation(rs) for _ in range(k)])


def rotations_twins(rs, angle):
    """Two rotations `angle` rad apart."""
    R = rand_rotation(rs)
    return np.stack((R, R @ rodrigues(angle * rand_axis(rs))))


def rotations_planar(rs):
    """The two-fold ambiguity of a planar scene: R and R diag(-1, -1, 1)."""
    R = rand_rotation(rs)
    return np.stack((R, R @ np.diag([-1.0, -1.0, 1.0])))


def rotations_near(rs, k, radius):
    """k rotations, every one within `radius` rad of a common one."""
    R = rand_rotation(rs)
    return np.stack([R @ rodrigues(radius * rs.uniform(0.2, 1.0) * rand_axis(rs)) for _ in range(k)])


def weights(rs, k, wmin):
    """Positive weights that sum to one (Z[9][9] = 1, as for a feasible SDP point).  k = 2: both >= wmin.  k > 2: drawn from
    [wmin, 1] and then normalised, so the smallest is at least wmin / (wmin + k - 1)."""
    if k == 1:
        return np.ones(1)
    if k == 2:
        a = rs.uniform(wmin, 1.0 - wmin)
        return np.array([a, 1.0 - a])
    w = rs.uniform(wmin, 1.0, size=k)
    return w / w.sum()


def plant_Z(Rs, w):
    """sum_i w_i z_i z_i^T as a 10x10, summed entry by entry (no BLAS: the same bits everywhere)."""
    Z = np.zeros((10, 10))
    for Ri, wi in zip(Rs, w):
        z = z_of(Ri)
        Z = Z + wi * np.outer(z, z)
    return 0.5 * (Z + Z.T)


def sym_noise(rs, scale):
    E = rs.normal(scale=scale, size=(10, 10))
    return 0.5 * (E + E.T)


def rand_B27(rs):
    """A 3x9 translation map (t = -B r), row-major, entries on a grid of 1/64 in [-2, 2]: exact in binary, |B|_inf > 1."""
    return rs.randint(-128, 129, size=27) / 64.0


def second_weight_for(Rs, lam2):
    """Weights (1 - w, w) of two planted rotations for which the second eigenvalue of Z is lam2 (bisection: it grows with w)."""
    lo, hi = 0.0, 0.5
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if np.linalg.eigvalsh(plant_Z(Rs, (1.0 - mid, mid)))[-2] < lam2:
            lo = mid
        else:
            hi = mid
    return np.array([1.0 - hi, hi])


def polish_Q(Rs, rs):
    """A cost whose zero-cost global minimisers include every planted rotation: Q = P M M^T P with P the projector off
    span{vec R_i}.  Returns the symmetric 9x9."""
    V = np.stack([vec(R) for R in Rs], axis=1)           # 9 x k
    Qb, _ = np.linalg.qr(V)
    P = np.eye(9) - Qb @ Qb.T
    M = rs.normal(size=(9, 12))
    Q = P @ M @ M.T @ P
    return 0.5 * (Q + Q.T)


# ---------------------------------------------------------------------------------------------------------- numpy facts
def eigenvalues(Z55):
    return np.linalg.eigvalsh(vech10_inv(Z55))


def np_rank(Z55):
    """The rank rule of cvxpnpl.py:502."""
    return int((eigenvalues(Z55) > RANK_TOL).sum())


def rank_margin(Z55):
    """Distance of the nearest eigenvalue from the rank threshold."""
    return float(np.abs(eigenvalues(Z55) - RANK_TOL).min())


def expected_count(rank):
    """Poses the recovery returns for a numpy rank (cvxpnpl.py:231, :504): 1 for rank 1, 2 or 4 above it, -1 for rank 0."""
    if rank <= 0:
        return -1
    if rank == 1:
        return 1
    return min(2 * ((rank + 1) // 2), 4)


def tangent_basis(R):
    """J = d vec(R exp([w]x)) / dw at w = 0: column k is vec(R [e_k]x).  9 x 3."""
    J = np.zeros((9, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        Ex = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        J[:, k] = vec(np.asarray(R) @ Ex)
    return J


def riemannian_hessian(Q, R):
    """3x3 Hessian of r^T Q r on SO(3) at R, when Q vec(R) = 0 (the curvature term then vanishes): 2 J^T Q J."""
    J = tangent_basis(R)
    return 2.0 * J.T @ np.asarray(Q) @ J


def hessian_cond(Q, Rs):
    """Largest condition number of the Riemannian Hessian over the planted rotations."""
    worst = 0.0
    for R in Rs:
        ev = np.linalg.eigvalsh(riemannian_hessian(Q, R))
        worst = max(worst, np.inf if ev[0] <= 0 else ev[-1] / ev[0])
    return worst


# -------------------------------------------------------------------------------------------------------------- metrics
def rot_err(R_out, R_planted):
    """max over planted R_i of min over returned R_j of |R_j - R_i|_F, and the matched j per planted i.
    R_out [n, 3, 3] (only the returned slots), R_planted [k, 3, 3].  NaN slots never match; no finite slot: inf."""
    R_out = np.asarray(R_out, dtype=np.float64).reshape(-1, 3, 3)
    R_planted = np.asarray(R_planted, dtype=np.float64).reshape(-1, 3, 3)
    if len(R_out) == 0:
        return np.inf, np.full(len(R_planted), -1)
    d = np.sqrt(((R_out[None] - R_planted[:, None]) ** 2).sum(axis=(2, 3)))  # [k, n]
    d = np.where(np.isnan(d), np.inf, d)
    match = d.argmin(axis=1)
    return float(d.min(axis=1).max()), match


def trans_err(t_out, B27, R_planted, match):
    """The translation twin: max over planted i of |t_j + B vec(R_i)|_inf for the matched j, scaled by max(1, |B|_inf)."""
    t_out = np.asarray(t_out, dtype=np.float64).reshape(-1, 3)
    B = np.asarray(B27, dtype=np.float64).reshape(3, 9)
    worst = 0.0
    for i, R in enumerate(np.asarray(R_planted).reshape(-1, 3, 3)):
        if match[i] < 0:
            return np.inf
        e = np.abs(t_out[match[i]] + B @ vec(R)).max()
        worst = max(worst, np.inf if np.isnan(e) else e)
    return float(worst / max(1.0, np.abs(B).sum(axis=1).max()))


def bound_unpolished(ref_err, k):
    """The rule for unpolished k = 2 / 4 problems: FACTOR * the reference's own error + FLOOR; the floor alone where the
    reference returns NaN; a k = 4 problem on which the reference is worse than DESIGN_BOUND is still held to DESIGN_BOUND."""
    if not np.isfinite(ref_err):
        return FLOOR
    if k == 4 and ref_err > DESIGN_BOUND:
        return DESIGN_BOUND
    return FACTOR * ref_err + FLOOR


# -------------------------------------------------------------------------------------------------------------- fixture
# class name -> (planted rotations per problem, problems).  The generator and the tests share this table.
CLASSES = {
    "k2_rand_w25": (2, 16), "k2_rand_w02": (2, 16),
    "k2_twin_05": (2, 16), "k2_twin_02": (2, 16), "k2_twin_01": (2, 16),
    "planar_eq": (2, 64), "planar_73": (2, 64),
    "k4_rand_w25": (4, 32), "k4_rand_w02": (4, 32), "k4_near": (4, 32),
    "k2_polish": (2, 16), "k4_polish": (4, 16), "k2_polish_noise": (2, 16), "k4_polish_noise": (4, 16),
    "r1_exact": (1, 16), "r1_pert": (1, 16),
    "r3": (3, 16), "r5": (5, 16), "r6": (6, 16),
    "thr_hi": (2, 16), "thr_lo": (2, 16),
}
UNPOLISHED_K2 = ("k2_rand_w25", "k2_rand_w02", "k2_twin_05", "k2_twin_02", "k2_twin_01", "planar_eq", "planar_73")
UNPOLISHED_K4 = ("k4_rand_w25", "k4_rand_w02", "k4_near")
POLISHED = ("k2_polish", "k4_polish", "k2_polish_noise", "k4_polish_noise")
RANK1 = ("r1_exact", "r1_pert")
ODD = ("r3", "r5", "r6")
THRESHOLD = ("thr_hi", "thr_lo")
COUNTED = UNPOLISHED_K2 + UNPOLISHED_K4 + POLISHED + RANK1 + THRESHOLD  # classes whose pose count follows the numpy rank rule


STORED_Z = ("k2_polish_noise", "k4_polish_noise", "r1_pert")  # Z carries noise; everywhere else Z = plant_Z(R, w) exactly


def complete_class(name, cls):
    """Add what follows from the stored arrays: Z55 of the exact classes and the reference's error against the planted truth."""
    if "Z55" not in cls:
        cls["Z55"] = np.stack([vech10(plant_Z(Rs, w)) for Rs, w in zip(cls["R"], cls["w"])])
    err = np.full(len(cls["R"]), np.nan)
    for i, (Rr, m) in enumerate(zip(cls["ref_R"], cls["ref_n"])):
        if np.isfinite(Rr[:m]).all():
            err[i] = rot_err(Rr[:m], cls["R"][i])[0]
    cls["ref_err"] = err
    return cls


@functools.lru_cache(maxsize=None)
def load_fixture(path=FIXTURE):
    """{class: {"Z55" [N,55], "R" [N,k,3,3], "w" [N,k], "B27" [N,27], "ref_R" [N,4,3,3] (NaN-padded), "ref_n" [N],
    "ref_err" [N] (NaN where the reference returns NaN), and "Q45" [N,45] for the polish classes}}.  Z55 of the classes
    without noise and ref_err are rebuilt from the stored arrays (complete_class).  Read once, shared by every test, read-only."""
    raw = np.load(path, allow_pickle=False)
    out = {}
    for name in CLASSES:
        out[name] = {}
        for key in raw.files:
            if key.startswith(name + "__"):
                out[name][key[len(name) + 2:]] = raw[key]
        for a in complete_class(name, out[name]).values():
            a.setflags(write=False)
    return out


def concat(names, fixture=None):
    """The problems of several classes in one batch: Z55 [n,55], B27 [n,27], Q45 [n,45] (zeros where a class has none) and
    (class, index) per problem."""
    fx = fixture or load_fixture()
    Z = np.concatenate([fx[c]["Z55"] for c in names])
    B = np.concatenate([fx[c]["B27"] for c in names])
    Q = np.concatenate([fx[c]["Q45"] if "Q45" in fx[c] else np.zeros((len(fx[c]["Z55"]), 45)) for c in names])
    who = [(c, i) for c in names for i in range(len(fx[c]["Z55"]))]
    return Z, B, Q, who


def judge(name, cls, cnt, R, t):
    """The truth rules for one class.  cnt [N], R [N,4,3,3], t [N,4,3]: what a recovery returned for the class's problems
    (with the class's Q45 where it has one, without a cost otherwise).  Asserts, and returns the figures:
    {"err": [N] rotation error against the planted truth, "terr": [N] its translation twin, "bound": [N]}."""
    k, n = CLASSES[name]
    err, terr, bound = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        if name in COUNTED:
            want = expected_count(np_rank(cls["Z55"][i]))
            assert cnt[i] == want, (name, i, int(cnt[i]), want)
        m = max(int(cnt[i]), 0)
        assert np.isnan(R[i, m:]).all() and np.isnan(t[i, m:]).all(), (name, i, "slots beyond n_poses are not NaN")
        # thr_lo: numpy rank 1, so one pose comes back, next to the dominant planted rotation; it and the reference's are
        # measured against that one.  r1_pert: the planted rotation is not the exact answer of the perturbed Z, but the
        # reference's distance from it (1e-5) still pins the rank-1 branch to FACTOR times itself.
        planted = cls["R"][i][:1] if name == "thr_lo" else cls["R"][i]
        ref_err = rot_err(cls["ref_R"][i, :cls["ref_n"][i]], planted)[0] if name == "thr_lo" else cls["ref_err"][i]
        err[i], match = rot_err(R[i, :m], planted)
        terr[i] = trans_err(t[i, :m], cls["B27"][i], planted, match)
        if name in POLISHED:
            bound[i] = POLISH_BOUND
        elif name in UNPOLISHED_K2 + UNPOLISHED_K4 + RANK1 + THRESHOLD:
            bound[i] = bound_unpolished(ref_err, 4 if name in UNPOLISHED_K4 else 2)
    held = np.isfinite(bound)
    worst = np.where(held, np.maximum(err, terr) / np.where(held, bound, 1.0), 0.0)
    i = int(worst.argmax())
    assert (worst <= 1.0).all(), (name, i, f"err {err[i]:.3e} terr {terr[i]:.3e} bound {bound[i]:.3e} reference {cls['ref_err'][i]:.3e}")
    return {"err": err, "terr": terr, "bound": bound}


def check_odd(name, cls, cnt, R, t):
    """Rank 3 / 5 / 6 (recorded only): counts are 2 or 4, every returned slot is a finite orthogonal matrix (to 1e-9) or NaN,
    slots beyond the count are NaN.  Returns how many planted poses are among the returned ones (to 1e-6)."""
    found = 0
    for i in range(len(cnt)):
        assert cnt[i] in (2, 4), (name, i, cnt[i])
        assert np.isnan(R[i, cnt[i]:]).all() and np.isnan(t[i, cnt[i]:]).all(), (name, i)
        for s in range(cnt[i]):
            if np.isnan(R[i, s]).any():
                assert np.isnan(R[i, s]).all() and np.isnan(t[i, s]).all(), (name, i, s)
            else:
                assert np.abs(R[i, s] @ R[i, s].T - np.eye(3)).max() < 1e-9 and np.isfinite(t[i, s]).all(), (name, i, s)
        d = np.sqrt(((R[i, None, :cnt[i]] - cls["R"][i][:, None]) ** 2).sum(axis=(2, 3)))
        found += int((np.where(np.isnan(d), np.inf, d).min(axis=1) < 1e-6).sum())
    return found


def figures(name, res, cls):
    """One line for the record: the worst errors of a class next to the reference's."""
    ref = cls["ref_err"]
    return (f"{name:16s} rot max {np.nanmax(res['err']):.2e} median {np.nanmedian(res['err']):.2e}  t max {np.nanmax(res['terr']):.2e}"
            f"  reference max {np.nanmax(ref):.2e} (NaN on {int(np.isnan(ref).sum())})")
