"""Independent reference of the robust reprojection refinement (cvxpnpl_amd/csrc/refine_robust_core.h), numpy only, no library code.

From tests/refine_reference.py it takes the residuals, their difference Jacobian in the public chart, expm_so3 and far_h.  Written here,
from the table of the issue: rho, rho', the cost  sum_k w_k rho(s_k),  the re-weighted step and the schedule restated on the robust cost.
``cost_gradient`` differentiates the cost by central differences of RHO ITSELF (long double, the public chart): it never uses rho', so a
library whose rho' does not belong to its rho cannot pass a stationarity check made with it.  One problem per call.

s_k is per correspondence: a point's squared pixel distance, a line's two squared end-point distances together.
"""
import numpy as np

import refine_reference as ref

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, COST_TOL = 1e-3, 1e-12, 1e12, 1e-12
LOSSES = ("l2", "huber", "cauchy")


def rho(loss, s, delta):
    s = np.asarray(s)
    if loss == "l2":
        return s
    d2 = delta * delta
    if loss == "huber":
        with np.errstate(invalid="ignore"):
            return np.where(s <= d2, s, 2.0 * delta * np.sqrt(s) - d2)
    if loss == "cauchy":
        return d2 * np.log1p(s / d2)
    raise ValueError(loss)


def rho_prime(loss, s, delta):
    s = np.asarray(s, float)
    if loss == "l2":
        return np.ones_like(s)
    d2 = delta * delta
    if loss == "huber":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s <= d2, 1.0, delta / np.sqrt(s))
    if loss == "cauchy":
        return 1.0 / (1.0 + s / d2)
    raise ValueError(loss)


def _split(data):
    """(correspondence arguments of ref.residuals without masks, mask_pts, mask_lines, weights_pts, weights_lines)"""
    d = dict(data)
    mp, ml, wp, wl = d.pop("mask_pts", None), d.pop("mask_lines", None), d.pop("weights_pts", None), d.pop("weights_lines", None)
    return d, mp, ml, wp, wl


def live_weights(**data):
    """(live points [n_p] bool, live lines [n_l] bool, weights of the points [n_p], of the lines [n_l], bad): live = mask byte absent or
    non-zero, for a line a != b, and weight != 0; bad = some record that its mask admits has a negative or non-finite weight."""
    d, mp, ml, wp, wl = _split(data)
    n_p = 0 if d.get("pts_2d") is None else len(d["pts_2d"])
    n_l = 0 if d.get("line_2d") is None else len(d["line_2d"])
    ap = np.ones(n_p, bool) if mp is None else np.asarray(mp) != 0
    al = np.ones(n_l, bool) if ml is None else np.asarray(ml) != 0
    wp = np.ones(n_p) if wp is None else np.asarray(wp, float)
    wl = np.ones(n_l) if wl is None else np.asarray(wl, float)
    with np.errstate(invalid="ignore"):
        bad = bool((ap & ~((wp >= 0) & np.isfinite(wp))).any() or (al & ~((wl >= 0) & np.isfinite(wl))).any())
        lp, ll = ap & (wp > 0) & np.isfinite(wp), al & (wl > 0) & np.isfinite(wl)
        if n_l:
            l2 = np.asarray(d["line_2d"])
            ll = ll & ~np.all(l2[:, 0] == l2[:, 1], axis=1)
    return lp, ll, wp, wl, bad


def _live_call(data):
    """data as ref.residuals takes it, the live selection passed as its masks"""
    d, *_ = _split(data)
    lp, ll, wp, wl, bad = live_weights(**data)
    return dict(d, mask_pts=lp.astype(np.uint8) if len(lp) else None, mask_lines=ll.astype(np.uint8) if len(ll) else None), lp, ll, wp, wl


def squares(K, R, t, **data):
    """(s over the live records: points then lines, their weights, the row -> record map of ref.residuals' vector, r, min depth)"""
    call, lp, ll, wp, wl = _live_call(data)
    r, zmin = ref.residuals(K, R, t, **call)
    n, m = int(lp.sum()), int(ll.sum())
    rows = np.concatenate([np.repeat(np.arange(n), 2), n + np.arange(m), n + np.arange(m)]).astype(int)   # (x, y) per point; e0 of every line, then e1
    s = np.zeros(n + m, dtype=r.dtype)
    np.add.at(s, rows, r * r)
    w = np.concatenate([wp[lp], wl[ll]])
    return s, w, rows, r, zmin


def cost(K, R, t, loss, delta, **data):
    s, w, _, _, zmin = squares(K, R, t, **data)
    return float((w * rho(loss, s, delta)).sum()), zmin


def robust_w_full(K, R, t, loss, delta, **data):
    """rho'(s_k) for EVERY record (points then lines), 0 where not live; and the number of live records with s_k <= delta^2; and s."""
    lp, ll, *_ = live_weights(**data)
    s, w, _, _, _ = squares(K, R, t, **data)
    out = np.zeros(len(lp) + len(ll))
    out[np.concatenate([lp, ll])] = rho_prime(loss, s, delta)
    n_in = int(len(s) if loss == "l2" else (s <= delta * delta).sum())
    return out, n_in, s


def lm_step(K, R, t, loss, delta, lam=LAMBDA0, h=1e-3, **data):
    """(d, A, g, J, r, omega per row): (A + lam diag A) d = -g with A = J^T diag(omega) J, g = J^T diag(omega) r, omega_k = w_k rho'(s_k)"""
    call, *_ = _live_call(data)
    s, w, rows, r, _ = squares(K, R, t, **data)
    J = ref.jacobian(K, R, t, h=h, **call)
    om = (w * rho_prime(loss, s, delta))[rows]
    A = J.T @ (om[:, None] * J)
    g = J.T @ (om * r)
    d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
    return d, A, g, J, r, om


def cost_gradient(K, R, t, loss, delta, h=1e-3, **data):
    """(d cost / d (w, tau) in the public chart by the sixth-order central difference of the COST in long double -- rho, never rho' --
    and the scale  sum over the rows of |J_row| |r_row| omega_row  it is judged against)"""
    ld = np.longdouble
    Kl, Rl, tl = np.asarray(K, ld), np.asarray(R, ld), np.asarray(t, ld)
    dl = {k: (np.asarray(v, ld) if v is not None and not k.startswith("mask") else v) for k, v in data.items()}

    def f(xi):
        s, w, _, _, _ = squares(Kl, ref.expm_so3(xi[:3]) @ Rl, tl + xi[3:], **dl)
        return (w * rho(loss, s, ld(delta))).sum()
    g = np.zeros(6)
    for k in range(6):
        e = np.zeros(6, ld)
        e[k] = h
        g[k] = float((45.0 * (f(e) - f(-e)) - 9.0 * (f(2 * e) - f(-2 * e)) + (f(3 * e) - f(-3 * e))) / (60.0 * h))
    _, _, _, J, r, om = lm_step(K, R, t, loss, delta, h=h, **data)
    return g, float((np.linalg.norm(J, axis=1) * np.abs(r) * om).sum())


def refine(K, R, t, loss="huber", delta=1.0, max_iters=30, step_tol=1e-10, h=1e-3, **data):
    """The schedule of refine_core.h on the robust cost, one problem.  Returns dict(R, t, cost (before, after), iters, status, n_live,
    history, rejected).  Statuses: 2 a non-finite pose or det R <= 0; 4 a bad weight (see live_weights); 3 fewer than 3 live records; 4 a
    live record behind the camera or with a non-finite number; otherwise 0 / 1."""
    R, t = np.array(R, float), np.array(t, float)
    lp, ll, wp, wl, bad = live_weights(**data)
    n_live = int(lp.sum() + ll.sum())
    skip = {"R": R, "t": t, "cost": (np.nan, np.nan), "iters": 0, "rejected": 0, "n_live": n_live, "history": []}
    if not np.all(np.isfinite(R)) or not np.all(np.isfinite(t)) or not np.linalg.det(R) > 0:
        return dict(skip, status=2)
    if bad:
        return dict(skip, status=4)
    if n_live < 3:
        return dict(skip, status=3)
    with np.errstate(invalid="ignore", over="ignore"):
        c, zmin = cost(K, R, t, loss, delta, **data)
    if not np.isfinite(c) or not zmin > 0:
        return dict(skip, status=4)
    cost0 = c
    lam, iters, status, hist, rejected = LAMBDA0, 0, 1, [c], 0
    while iters < max_iters:
        iters += 1
        d = lm_step(K, R, t, loss, delta, lam, h=h, **data)[0]
        Rn, tn = ref.expm_so3(d[:3]) @ R, t + d[3:]
        cn, zn = cost(K, Rn, tn, loss, delta, **data)
        small = np.linalg.norm(d) <= step_tol * (1.0 + np.linalg.norm(t))
        floor = lam <= LAMBDA0 and abs(cn - c) <= COST_TOL * c
        if zn > 0 and cn <= c:
            R, t, c = Rn, tn, cn
            hist.append(c)
            lam = max(lam / 10.0, LAMBDA_MIN)
            if small or floor:
                status = 0
                break
        elif zn > 0 and ((small and lam <= LAMBDA0) or floor):
            status = 0
            break
        else:
            rejected += 1
            lam *= 10.0
            if lam > LAMBDA_MAX:
                break
    return {"R": R, "t": t, "cost": (cost0, c), "iters": iters, "status": status, "n_live": n_live, "history": hist, "rejected": rejected}
