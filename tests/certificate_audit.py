"""An independent bracket  L <= p* <= U  of the relaxation's optimum, and the audit of a certificate against it.

Plain helper module (imported like grad_reference.py).  It uses numpy, the CPU oracle (oracle/, pinned to the reference by the
golden files), the golden fixtures, and cvxpnpl_amd.synth for making inputs.  Nothing else of the product and nothing of
tests/hostsim enters it: what is audited comes in as plain arrays (R, t, cost, dobj).

The SDP (cvxpnpl.py:454-489):  p* = min <Q, Z>  s.t.  <A_i, Z> = b_i,  Z >= 0,  Q = blkdiag(A^T A, 0).  On vech(Z):
c = vech(Q, 2) so that c . vech(Z) = <Q, Z>, and the equality rows are the REFERENCE'S OWN rows g4_A[:22], g4_b[:22] of
tests/golden/reference_vectors.npz (rc variant: the 16 zero-cone rows of oracle.sdp_constraints_rc(), pinned bit for bit by
reference_vectors_rc.npz).

  L   the oracle's SCS port returns multipliers y of the equalities that are only approximately dual feasible; the bound is made
      rigorous here:  S = unvech(c + A_eq^T y)  (diagonal as is, off-diagonals halved),  L = -b_eq^T y + 4 min(0, lambda_min(S)).
      For every feasible Z:  <Q,Z> = <S,Z> - b_eq^T y >= lambda_min(S) tr Z - b_eq^T y,  and tr Z = 4.  The two facts this rests on
      are asserted from the rows themselves when they are loaded (_check_rows).
  U   ||A r_o||^2 in numpy.longdouble at the oracle's converged pose: any rotation is primal feasible (z = [vec R; 1], Z = z z^T),
      so this is an upper bound whatever the oracle did.  Where the oracle has no finite pose (exactly two-fold ambiguous scenes:
      it divides by a ~0 eigenvector entry) the rotations nearest to the top eigenvectors of its Z and to
      their sum and difference, polished by a plain Gauss-Newton of this module, stand in -- still rotations, still upper bounds.

FLOOR: the float64 floor of the reported cost, measured in the reference's arithmetic (measure_cost_floor); k_of(cls) is the k of
the assertions A1-A3 derived from it.  The cases every audit file uses are made here (parity_case ... rc_case) so that the floor is
measured on exactly the problems that are audited.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U64 = 2.0 ** -52
EPS = 1e-9  # the product's default certificate tolerance (reference default eps)

# Float64 floor of the reported cost in the REFERENCE'S arithmetic: the worst  |r^T (C^T C - (N^T C)^T B) r - cost_ld(R)| / (u tr A^T A)
# with numpy float64 at the oracle's pose (measure_cost_floor), over the first 64 problems (24 for N = 4) of every audited case,
# measured on the CPU (tests/test_certificate_audit.py::test_cost_floor_constants_hold re-measures them):
#   near    11.9   the eight CASES of test_gpu_parity.py and the rc batch (worst: 20 points + 9 lines; the others 3.9 .. 8.6)
#   planar  125    planar scenes (general frame: random plane and offset; canonical frame 20.2)
#   far     7.52   world origin 1e3 scene sizes away, with C, N built from the 3D points taken about their centroid (the cost does
#                  not depend on the centre; still numpy float64 and the oracle's rows, nothing of the product).  Uncentred, as the
#                  reference forms them, the Schur form cancels eight digits there and the same measurement gives 1.18e8 u tr Q --
#                  a tolerance of 8e-7 tr Q, above eps, under which A1-A3 would be vacuous; recorded, not used.  (The reference's own
#                  explicit A, against which the cost is held, is itself 8.2 u tr Q from the A of the centred points.)
#   large   9.45   N = 2 000 points
# The kernel gets K_MARGIN = 32 x the worst floor of its class: another summation order and another centre, the same conditioning.
FLOOR = {"near": 12.0, "planar": 126.0, "far": 7.6, "large": 9.5}   # the figures above, rounded up
K_MARGIN = 32.0


def k_of(cls):
    return K_MARGIN * FLOOR[cls]


_ROWS = {}
_BRACKETS = {}


def reference_A_B(orc, d, i, n_p, n_l):
    """A (m x 9), B (3 x 9) of problem i the way cvxpnpl.pnp / pnl / pnpl build them (cvxpnpl.py:545-549, :577-580, :619-624)"""
    Cm, N = reference_C_N(orc, d, i, n_p, n_l)
    B, A = orc.eliminate(Cm, N)
    return A, B


def reference_C_N(orc, d, i, n_p, n_l):
    Cs, Ns = [], []
    K = d["K"] if d["K"].ndim == 2 else d["K"][i]
    if n_p:
        (c1, c2, c3), (n1, n2, n3) = orc.point_constraints(d["pts_2d"][i], d["pts_3d"][i], K)
        Cs += [c1, c2, c3]
        Ns += [n1, n2, n3]
    if n_l:
        cl, nl = orc.line_constraints(d["line_2d"][i], d["line_3d"][i], K)
        Cs.append(cl)
        Ns.append(nl)
    return np.vstack(Cs), np.vstack(Ns)


def vec(R):
    """r = vec(R), column-major: r[3 j + i] = R[i][j] (the reference's r; t = -B r)"""
    return np.asarray(R).T.reshape(9)


def vech_zz(R):
    """vech(z z^T), z = [vec R; 1], in the reference's packing (columns of the lower triangle, no scaling)"""
    z = np.concatenate([vec(R), [1.0]])
    return oracle.vech10(np.outer(z, z), 1.0)


def unvech_half(v):
    """the symmetric matrix S with  v . vech(Z) = <S, Z>  (diagonal as is, off-diagonals halved)"""
    M = oracle.vech10_inv(v)
    return 0.5 * (M + np.diag(np.diag(M)))


def random_rotation(rs):
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    a, b, c, e = q
    return np.array([[a * a + b * b - c * c - e * e, 2 * (b * c - a * e), 2 * (b * e + a * c)],
                     [2 * (b * c + a * e), a * a - b * b + c * c - e * e, 2 * (c * e - a * b)],
                     [2 * (b * e - a * c), 2 * (c * e + a * b), a * a - b * b - c * c + e * e]])


def _check_rows(Aeq, beq):
    """What the lower bound rests on, from the rows themselves: a rotation's vech(z z^T) satisfies them to 1e-14 and has trace 4,
    and the rows force trace 4 on EVERY feasible Z (the identity's vech lies in their row space, with right-hand side 4)."""
    rs = np.random.RandomState(5)
    I55 = oracle.vech10(np.eye(10), 1.0)
    for _ in range(8):
        R = random_rotation(rs)
        x = vech_zz(R)
        assert np.abs(Aeq @ x - beq).max() <= 1e-14, np.abs(Aeq @ x - beq).max()
        assert abs(I55 @ x - 4.0) <= 1e-14
        Qm = rs.standard_normal((10, 10))
        Qm = Qm + Qm.T
        z = np.concatenate([vec(R), [1.0]])
        assert abs(oracle.vech10(Qm, 2.0) @ x - z @ Qm @ z) <= 1e-13 * np.abs(Qm).sum()   # c . vech(Z) = <Q, Z>
        assert abs(np.sum(unvech_half(oracle.vech10(Qm, 2.0)) * np.outer(z, z)) - z @ Qm @ z) <= 1e-13 * np.abs(Qm).sum()
    w, res, *_ = np.linalg.lstsq(Aeq.T, I55, rcond=None)
    assert np.abs(Aeq.T @ w - I55).max() <= 1e-13 and abs(w @ beq - 4.0) <= 1e-13     # tr Z = 4 follows from the rows


def equality_rows(rc=False):
    """(A_eq, b_eq): the reference's equality rows on vech(Z) -- 22 from the golden file, or the 16 of the rc variant"""
    if rc not in _ROWS:
        if rc:
            Ad, b = oracle.sdp_constraints_rc()
            g = np.load(os.path.join(_GOLDEN, "reference_vectors_rc.npz"), allow_pickle=False)
            assert np.array_equal(Ad, g["rc_A"]) and np.array_equal(b, g["rc_b"])
            Aeq, beq = g["rc_A"][:16].copy(), g["rc_b"][:16].copy()
        else:
            g = np.load(os.path.join(_GOLDEN, "reference_vectors.npz"), allow_pickle=False)
            Aeq, beq = g["g4_A"][:22].copy(), g["g4_b"][:22].copy()
        _check_rows(Aeq, beq)
        _ROWS[rc] = (Aeq, beq)
    return _ROWS[rc]


def cost_ld(A, R):
    """||A vec(R)||^2 in numpy.longdouble"""
    v = np.asarray(A, dtype=np.longdouble) @ np.asarray(vec(R), dtype=np.longdouble)
    return v @ v


def cost_f64_schur(Cm, N, R):
    """r^T (C^T C - (N^T C)^T B) r in numpy float64, B = (N^T N)^-1 N^T C: the quantity the kernels report, in the reference's
    arithmetic (explicit C, N; numpy's summation order).  Its distance from cost_ld is the float64 floor of that quantity."""
    NtC = N.T @ Cm
    B = np.linalg.solve(N.T @ N, NtC)
    r = vec(R)
    return float(r @ ((Cm.T @ Cm - NtC.T @ B) @ r))


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def polish(A, R, steps=40):
    """Gauss-Newton of ||A vec(R)||^2 on SO(3) (left perturbation exp([w]x) R) from the rotation nearest to R.  Whatever it
    returns is a rotation, hence an upper bound; how good a bound shows in the bracket's width."""
    U_, _, Vt = np.linalg.svd(R)
    R = U_ @ np.diag([1, 1, np.linalg.det(U_ @ Vt)]) @ Vt
    for _ in range(steps):
        J = np.stack([A @ vec(_hat(g) @ R) for g in np.eye(3)], 1)
        w = -np.linalg.lstsq(J, A @ vec(R), rcond=None)[0]
        th = np.linalg.norm(w)
        if not np.isfinite(th) or th < 1e-16:
            break
        Kx = _hat(w / th)
        U_, _, Vt = np.linalg.svd((np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ R)
        R = U_ @ Vt
    return R


def _candidates_from_Z(A, x):
    """rotations near the top eigenvectors of the oracle's Z (and their sum / difference), polished"""
    lam, V = np.linalg.eigh(oracle.vech10_inv(x))
    out = []
    for v in (V[:, -1], V[:, -2], V[:, -1] + V[:, -2], V[:, -1] - V[:, -2]):
        for s in (1.0, -1.0):
            M = s * v[:9].reshape(3, 3).T
            U_, _, Vt = np.linalg.svd(M)
            if np.linalg.det(U_ @ Vt) > 0:
                out.append(polish(A, U_ @ Vt))
    return out


def bracket(A, B, rc=False):
    """dict(L, U, w, R_o, trQ, y, lam_min) for one problem.  L, U as in the module docstring; R_o the rotation U was evaluated at."""
    Aeq, beq = equality_rows(rc)
    Q = np.zeros((10, 10))
    Q[:9, :9] = A.T @ A
    c = oracle.vech10(Q, 2.0)
    sol = (oracle.scs_solve_rc if rc else oracle.scs_solve)(c, eps=1e-11, max_iters=200000)
    y = sol["y"][:len(beq)]
    lam_min = float(np.linalg.eigvalsh(unvech_half(c + Aeq.T @ y))[0]) if np.isfinite(y).all() else -np.inf
    L = -float(beq @ y) + 4.0 * min(0.0, lam_min) if np.isfinite(lam_min) else -np.inf
    poses, info = (oracle.solve_relaxation_rc if rc else oracle.solve_relaxation)(A, B, eps=1e-11, max_iters=200000)
    cands = [R for R, _ in poses if np.isfinite(R).all() and abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12]
    if not cands or len(poses) > 1:
        cands += _candidates_from_Z(A, np.array(info.x[:]))
    costs = [cost_ld(A, R) for R in cands]
    k = int(np.argmin(costs)) if costs else -1
    U = costs[k] if costs else np.longdouble(np.inf)
    return {"L": L, "U": U, "w": float(U - L), "R_o": cands[k] if costs else None, "trQ": float(np.trace(Q)), "y": y, "lam_min": lam_min,
            "n_poses": len(poses), "scs_iters": sol["info"]["iter"]}


def case_brackets(key, d, n_p, n_l, idx, rc=False, ab=None):
    """brackets (with A, B) of problems idx of a case, computed once per key on a pool of at most 16 threads (ctypes releases the
    GIL).  ab(i) -> (A, B) replaces the correspondences d for problems given by explicit matrices (the cost seam)."""
    store = _BRACKETS.setdefault((key, rc), {})
    todo = [int(i) for i in idx if int(i) not in store]
    if todo:
        oracle.lib()
        equality_rows(rc)

        def one(i):
            A, B = ab(i) if ab is not None else reference_A_B(oracle, d, i, n_p, n_l)
            b = bracket(A, B, rc)
            b["A"], b["B"] = A, B
            return i, b

        with ThreadPoolExecutor(max_workers=16) as ex:
            for i, b in ex.map(one, todo):
                store[i] = b
    return store


class AuditFailure(AssertionError):
    pass


def audit_one(b, R, t, cost, dobj, k, eps=EPS):
    """Assertions A0-A3 for one problem the product calls certified.  b: its bracket (with A, B).  Returns
    dict(judged, over=dobj - min(U, cost_ld), gap=cost_ld - L); raises AuditFailure naming the assertion."""
    A, B = b["A"], b["B"]
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    tol = k * U64 * b["trQ"]
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(cost) and np.isfinite(dobj)):
        raise AuditFailure(f"A0 non-finite output: cost {cost} dobj {dobj}")
    if not np.abs(R @ R.T - np.eye(3)).max() <= 1e-12:
        raise AuditFailure(f"A0 R R^T - I = {np.abs(R @ R.T - np.eye(3)).max():.3e}")
    if not np.linalg.det(R) > 0:
        raise AuditFailure("A0 det R <= 0")
    if not np.abs(t + B @ vec(R)).max() <= 1e-9 * max(1.0, np.abs(t).max()):
        raise AuditFailure(f"A0 t + B r = {np.abs(t + B @ vec(R)).max():.3e}")
    c_ld = cost_ld(A, R)
    if not abs(float(np.longdouble(cost) - c_ld)) <= tol:
        raise AuditFailure(f"A1 cost {cost!r} vs ||A r||^2 {float(c_ld)!r}: off by {float(np.longdouble(cost) - c_ld):.3e}, allowed {tol:.3e}")
    over = float(np.longdouble(dobj) - min(b["U"], c_ld))
    if not over <= tol:
        raise AuditFailure(f"A2 dobj exceeds a primal-feasible value by {over:.3e} (allowed {tol:.3e}): not a lower bound")
    gap = float(c_ld - np.longdouble(b["L"]))
    judged = b["w"] <= eps / 10
    if judged and not gap <= eps + tol:
        raise AuditFailure(f"A3 ||A r||^2 - L = {gap:.3e} > eps = {eps:.1e} (+ {tol:.1e}); bracket width {b['w']:.2e}")
    return {"judged": bool(judged), "over": over, "gap": gap, "w": b["w"], "a1": abs(float(np.longdouble(cost) - c_ld)) / (U64 * b["trQ"])}


def audit_batch(brackets, r, idx, k, eps=EPS, max_left_out=0.0, label=""):
    """audit_one over problems idx of a result dict r (R, t, cost[:, 0], cost[:, 1]).  Returns the summary
    dict(n, left_out, worst_over, worst_gap); asserts the cap on the share A3 could not judge."""
    n = left = 0
    worst_over, worst_gap, worst_a1 = -np.inf, -np.inf, 0.0
    for i in idx:
        i = int(i)
        try:
            a = audit_one(brackets[i], r["R"][i], r["t"][i], r["cost"][i, 0], r["cost"][i, 1], k, eps)
        except AuditFailure as e:
            raise AuditFailure(f"{label} problem {i}: {e}") from None
        n += 1
        left += not a["judged"]
        worst_over = max(worst_over, a["over"])
        worst_a1 = max(worst_a1, a["a1"])
        if a["judged"]:
            worst_gap = max(worst_gap, a["gap"])
    assert left <= max_left_out * n + 1e-9, f"{label}: A3 could not judge {left} of {n} problems (cap {max_left_out:.0%})"
    s = {"n": n, "left_out": left, "worst_over": worst_over, "worst_gap": worst_gap, "worst_a1": worst_a1}
    print(f"audit {label}: {n} audited, {left} left out by A3, worst dobj - min(U, cost_ld) {worst_over:.3e}, worst cost_ld - L {worst_gap:.3e}, "
          f"worst |cost - cost_ld| {worst_a1:.1f} u tr Q (k = {k:g})")
    return s


def measure_cost_floor(d, n_p, n_l, idx, key, rc=False, centred=False):
    """max over idx of |cost_f64_schur - cost_ld| / (u tr A^T A) at the oracle's pose (R_o of the bracket); centred: C, N from the
    3D records taken about their centroid (cost_ld stays that of the reference's uncentred A)"""
    br = case_brackets(key, d, n_p, n_l, idx, rc)
    dd = d
    if centred:
        dd = dict(d)
        P = [d[k].reshape(len(d[k]), -1, 3) for k, m in (("pts_3d", n_p), ("line_3d", n_l)) if m]
        c = np.concatenate(P, axis=1).mean(axis=1)
        if n_p:
            dd["pts_3d"] = d["pts_3d"] - c[:, None, :]
        if n_l:
            dd["line_3d"] = d["line_3d"] - c[:, None, None, :]
    worst = 0.0
    for i in idx:
        b = br[int(i)]
        if b["R_o"] is None:
            continue
        Cm, N = reference_C_N(oracle, dd, int(i), n_p, n_l)
        worst = max(worst, abs(float(np.longdouble(cost_f64_schur(Cm, N, b["R_o"])) - cost_ld(b["A"], b["R_o"]))) / (U64 * b["trQ"]))
    return worst


# ------------------------------------------------------------------ the audited cases (inputs only: cvxpnpl_amd.synth)

def n_audit(n_p, n_l):
    """problems audited per case: the first 64, 24 for minimal problems (3.5 s of oracle each)"""
    return 24 if n_p + n_l <= 4 else 64


def parity_case(n_p, n_l, sigma, batch):
    """the inputs of test_gpu_parity.CASES"""
    from cvxpnpl_amd import synth

    return synth.make_pnpl(batch, n_p, n_l, sigma, seed=200 + n_p + 7 * n_l)


def planar_case(general, batch=64):
    from cvxpnpl_amd import synth

    return synth.make_planar_pnp(batch, 10, 0.5, seed=21, general=general)


def far_case(batch=64):
    """ten points, 1 px noise, the world origin ~1e3 scene sizes from the scene (the 'offset' scenes of tools/fuzz_hard.py)"""
    from cvxpnpl_amd import synth

    d = synth.make_pnp(batch, 10, 0.0, seed=31)
    rs = np.random.RandomState(32)
    c = rs.normal(size=(batch, 1, 3)) * 1e3
    d["pts_3d"] = d["pts_3d"] + c
    d["t_gt"] = d["t_gt"] - np.einsum("bij,bj->bi", d["R_gt"], c[:, 0])
    d["pts_2d"] = synth.project(d["pts_3d"], d["K"], d["R_gt"], d["t_gt"]) + rs.normal(scale=1.0, size=d["pts_2d"].shape)
    return d


def large_case(batch=16):
    from cvxpnpl_amd import synth

    d = synth.make_pnp(batch, 2000, 1.0, seed=2000)
    # the same images of a scene 1/16 the size (an exact scaling): tr A^T A = 1.33 instead of 341.  The oracle's stopping rule is
    # relative to |c|, so at 341 its multipliers leave brackets up to 1.9e-9 wide (7 of 16 above eps / 10, noise-free scenes
    # included); eps is absolute in the units of the cost.
    d["pts_3d"] = d["pts_3d"] / 16.0
    d["t_gt"] = d["t_gt"] / 16.0
    return d


def ipm_case(n_p):
    """(inputs, problems audited) of the interior-point tests: cases whose every problem the oracle alone brackets (N = 5, 6)"""
    from cvxpnpl_amd import synth

    if n_p == 4:
        return parity_case(4, 0, 1.0, 64), 24
    if n_p == 5:
        return synth.make_pnp(64, 5, 1.0, seed=205), 64
    return synth.make_pnp(256, 6, 2.0, seed=306), 160


def rc_case(batch=64):
    from cvxpnpl_amd import synth

    return synth.make_pnp(batch, 10, 1.0, seed=77)


def pack_upper(Q):
    """9 x 9 symmetric -> 45: the upper triangle row by row (the d_Q45 layout of the cost seam)"""
    return np.array([Q[a, b] for a in range(9) for b in range(a, 9)])


def certified(r):
    """problems the product calls certified: status CERTIFIED, or RANK_GT1 with a finite dobj (a certified twin pair, A4)"""
    return (r["status"] == 0) | ((r["status"] == 1) & np.isfinite(r["cost"][:, 1]))
