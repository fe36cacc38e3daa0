"""Independent reference of the reprojection refinement (cvxpnpl_amd/csrc/refine_core.h), numpy only.

It shares no code with the library: the residuals are written straight from their definition, the Jacobian is taken by central
differences in the PUBLIC chart  R' = exp([w]x) R, t' = t + tau  (the library works in a scene-centred chart and has analytic rows), the
Levenberg-Marquardt schedule is restated here, and (J^T J)^-1 is numpy's.  One problem per call.
"""
import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, COST_TOL = 1e-3, 1e-12, 1e12, 1e-12


def expm_so3(w):
    th = np.sqrt(w @ w)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th**2 * W @ W


def _pix(K, R, t, X):
    Y = X @ R.T + t
    h = Y @ K.T
    return h[:, :2] / h[:, 2:3], Y[:, 2]


def live_sets(pts_2d, line_2d, mask_pts=None, mask_lines=None):
    """Boolean selections of the live points and lines: mask byte absent or non-zero; a line with coincident 2D samples is not live."""
    n_p = 0 if pts_2d is None else len(pts_2d)
    n_l = 0 if line_2d is None else len(line_2d)
    lp = np.ones(n_p, bool) if mask_pts is None else np.asarray(mask_pts) != 0
    ll = np.ones(n_l, bool) if mask_lines is None else np.asarray(mask_lines) != 0
    if n_l:
        l2 = np.asarray(line_2d)
        with np.errstate(invalid="ignore"):
            ll = ll & ~np.all(l2[:, 0] == l2[:, 1], axis=1)
    return lp, ll


def residuals(K, R, t, pts_2d=None, pts_3d=None, line_2d=None, line_3d=None, mask_pts=None, mask_lines=None):
    """(r, min depth) over the live correspondences: points give pi(K (R X + t)) - x, lines the signed distances of both projected end
    points from the normalised image line through the two 2D samples."""
    lp, ll = live_sets(pts_2d, line_2d, mask_pts, mask_lines)
    out, depth = [], [np.inf]
    if lp.any():
        uv, z = _pix(K, R, t, np.asarray(pts_3d)[lp])
        out.append((uv - np.asarray(pts_2d)[lp]).ravel())
        depth.append(z.min())
    if ll.any():
        l2, l3 = np.asarray(line_2d)[ll], np.asarray(line_3d)[ll]
        a = np.concatenate([l2[:, 0], np.ones((len(l2), 1))], 1)
        b = np.concatenate([l2[:, 1], np.ones((len(l2), 1))], 1)
        l = np.cross(a, b)
        l = l / np.hypot(l[:, 0], l[:, 1])[:, None]
        for e in (0, 1):
            uv, z = _pix(K, R, t, l3[:, e])
            out.append(l[:, 0] * uv[:, 0] + l[:, 1] * uv[:, 1] + l[:, 2])
            depth.append(z.min())
    return (np.concatenate(out) if out else np.zeros(0)), min(depth)


def jacobian(K, R, t, h=1e-3, **data):
    """d r / d (w, tau) at (R, t) in the public chart, by the sixth-order central difference (steps h, 2h, 3h) of the residuals evaluated
    in numpy's long double: truncation ~ h^6 (1e-18 of the entries at the default), rounding ~ eps_long / h (1e-16 of them where long
    double is the 80-bit format, 1e-13 where it is float64), so that the covariance bound of the tests is not spent on the reference."""
    ld = np.longdouble
    K, R, t = np.asarray(K, ld), np.asarray(R, ld), np.asarray(t, ld)
    data = {k: (np.asarray(v, ld) if v is not None and not k.startswith("mask") else v) for k, v in data.items()}

    def f(xi):
        return residuals(K, expm_so3(xi[:3]) @ R, t + xi[3:], **data)[0]
    cols = []
    for k in range(6):
        e = np.zeros(6, ld)
        e[k] = h
        cols.append((45.0 * (f(e) - f(-e)) - 9.0 * (f(2 * e) - f(-2 * e)) + (f(3 * e) - f(-3 * e))) / (60.0 * h))
    return np.stack(cols, 1).astype(np.float64)


def far_h(**data):
    """The difference step for a scene far from the world origin: 1e-3 / (1 + max |X| over the live 3D records).  A rotation of h about
    the world origin moves a point at distance |X| by h |X|: with the fixed 1e-3 and points 100 units out, the residuals are sampled over
    a range on which the sixth-order formula no longer holds (the reference then reports a next step of 3.6e-3 from a converged pose)."""
    lp, ll = live_sets(data.get("pts_2d"), data.get("line_2d"), data.get("mask_pts"), data.get("mask_lines"))
    big = 0.0
    with np.errstate(invalid="ignore"):
        if lp.any():
            big = max(big, float(np.abs(np.asarray(data["pts_3d"], float)[lp]).max()))
        if ll.any():
            big = max(big, float(np.abs(np.asarray(data["line_3d"], float)[ll]).max()))
    return 1e-3 / (1.0 + big)


def live_data_finite(**data):
    """True when every number of a live record (its 2D and its 3D half) is finite."""
    lp, ll = live_sets(data.get("pts_2d"), data.get("line_2d"), data.get("mask_pts"), data.get("mask_lines"))
    ok = True
    if lp.any():
        ok = ok and np.isfinite(np.asarray(data["pts_2d"], float)[lp]).all() and np.isfinite(np.asarray(data["pts_3d"], float)[lp]).all()
    if ll.any():
        ok = ok and np.isfinite(np.asarray(data["line_2d"], float)[ll]).all() and np.isfinite(np.asarray(data["line_3d"], float)[ll]).all()
    return bool(ok)


def lm_step(K, R, t, lam=LAMBDA0, h=1e-3, **data):
    """The step the schedule takes from (R, t) at damping lam: (J^T J + lam diag(J^T J)) d = -J^T r.  Returns (d, J^T J, r)."""
    r, _ = residuals(K, R, t, **data)
    J = jacobian(K, R, t, h=h, **data)
    A = J.T @ J
    d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -J.T @ r)
    return d, A, r


def refine(K, R, t, max_iters=30, step_tol=1e-10, h=1e-3, **data):
    """The schedule of refine_core.h on one problem.  Returns dict(R, t, cost (before, after), iters, status, history of costs, rejected:
    the number of rejected trials, behind_trials: those of them whose trial pose had a live record at depth <= 0).  A pose that is not
    refined (status >= 2) is the input pose; a non-finite number in a live record is status 4, as a record behind the camera is."""
    R, t = np.array(R, float), np.array(t, float)
    with np.errstate(invalid="ignore", over="ignore"):
        r, zmin = residuals(K, R, t, **data)
    skip = {"R": R, "t": t, "cost": (np.nan, np.nan), "iters": 0, "rejected": 0, "behind_trials": 0}
    lp, ll = live_sets(data.get("pts_2d"), data.get("line_2d"), data.get("mask_pts"), data.get("mask_lines"))
    if not np.all(np.isfinite(R)) or not np.all(np.isfinite(t)) or not np.linalg.det(R) > 0:
        return dict(skip, status=2)
    if lp.sum() + ll.sum() < 3:
        return dict(skip, status=3)
    if not live_data_finite(**data) or not zmin > 0:
        return dict(skip, status=4)
    cost0 = cost = float(r @ r)
    lam, iters, status, hist, rejected, behind = LAMBDA0, 0, 1, [cost], 0, 0
    while iters < max_iters:
        iters += 1
        d, _, _ = lm_step(K, R, t, lam, h=h, **data)
        Rn, tn = expm_so3(d[:3]) @ R, t + d[3:]
        rn, zn = residuals(K, Rn, tn, **data)
        small = np.linalg.norm(d) <= step_tol * (1.0 + np.linalg.norm(t))
        floor = lam <= LAMBDA0 and abs(rn @ rn - cost) <= COST_TOL * cost   # the two costs agree to their rounding
        if zn > 0 and rn @ rn <= cost:
            R, t, cost = Rn, tn, float(rn @ rn)
            hist.append(cost)
            lam = max(lam / 10.0, LAMBDA_MIN)
            if small or floor:
                status = 0
                break
        elif zn > 0 and ((small and lam <= LAMBDA0) or floor):
            status = 0
            break
        else:
            rejected += 1
            behind += int(not zn > 0)
            lam *= 10.0
            if lam > LAMBDA_MAX:
                break
    return {"R": R, "t": t, "cost": (cost0, cost), "iters": iters, "status": status, "history": hist, "rejected": rejected, "behind_trials": behind}


def covariance(K, R, t, sigma2, h=1e-3, **data):
    """sigma2 (J^T J)^-1 at (R, t) in the public chart, and J^T J itself."""
    J = jacobian(K, R, t, h=h, **data)
    A = J.T @ J
    return sigma2 * np.linalg.inv(A), A
