"""The DEFINITION of the gradient of a robustly refined pose, in torch float64 autograd on the CPU -- what
tests/test_refine_robust_grad_host.py holds cvxpnpl_refine_robust_vjp_batch_host (csrc/refine_robust_vjp_core.h, the source of the
kernels) against.  Nothing is imported from cvxpnpl_amd and no formula of the core is restated: the residuals are written from the
definition of DESIGN.md section 15 with torch.matrix_exp, rho from the table of section 17 ALONE --

    l2  rho = s;    huber  rho = s for s <= delta^2, 2 delta sqrt(s) - delta^2 above;    cauchy  rho = delta^2 log1p(s / delta^2)

-- and rho', rho'' are never typed in: the cost is F = 1/2 sum_k w_k rho(s_k), s_k the squared residuals of record k (both steps), its
gradient g and Hessian H in the chart xi = (w, tau) come from double backward, the upstream covector b is the gradient at xi = 0 of
<G_R, R(xi)> + <g_t, t(xi)>, and

    dL/d(theta, w) = -(dg/d(theta, w))^T H^-1 b = -d/d(theta, w) (g . psi),  psi = H^-1 b held fixed.

Two charts, as in tests/refine_grad_reference.py: the one centred on the unweighted mean of the 3D records is the truth, its
disagreement with the plain chart is the reference's own noise floor.  variant="struck" strikes the rho'' term everywhere -- rho' is
held constant where g is differentiated, the forward iteration's Triggs form -- the shortcut the tests must tell apart.  The module
carries a Newton polish of its own (full Hessian, centred chart)."""
import numpy as np
import torch

F64 = torch.float64
NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d", "weights_pts", "weights_lines")
LOSSES = ("l2", "huber", "cauchy")


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=F64)


def hat(w):
    z = torch.zeros((), dtype=F64)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def pose_of(xi, R, t, c):
    """The public pose (R', t') of the chart point xi about c (c = 0: the plain chart)."""
    R1 = torch.matrix_exp(hat(xi[:3])) @ R
    return R1, R @ c + t + xi[3:] - R1 @ c


def residuals(R, t, K, pts_2d=None, pts_3d=None, line_2d=None, line_3d=None):
    """[n_p + n_l, 2]: the two residuals of every record, points first (u - x, v - y), then both end points of every line."""
    out = []

    def pix(X):
        h = (X @ R.T + t) @ K.T
        return h[..., :2] / h[..., 2:]

    if pts_3d is not None and len(pts_3d):
        out.append(pix(pts_3d) - pts_2d)
    if line_3d is not None and len(line_3d):
        a, b = line_2d[:, 0], line_2d[:, 1]
        one = torch.ones(len(a), 1, dtype=F64)
        l = torch.linalg.cross(torch.cat([a, one], 1), torch.cat([b, one], 1))
        l = l / torch.hypot(l[:, 0], l[:, 1])[:, None]
        uv = pix(line_3d)                                            # [n, 2, 2]
        out.append(l[:, None, 0] * uv[..., 0] + l[:, None, 1] * uv[..., 1] + l[:, None, 2])
    return torch.cat(out)


def rho(loss, s, delta):
    """The table of DESIGN.md section 17."""
    d2 = delta * delta
    if loss == "l2":
        return s
    if loss == "huber":
        above = torch.where(s <= d2, torch.full_like(s, d2), s)     # (the square root is never taken, nor differentiated, at 0)
        return torch.where(s <= d2, s, 2.0 * delta * torch.sqrt(above) - d2)
    if loss == "cauchy":
        return d2 * torch.log1p(s / d2)
    raise ValueError(loss)


def centre_of(pts_3d=None, line_3d=None):
    rows = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pts_3d, line_3d) if x is not None and len(x)]
    return np.concatenate(rows).mean(0)


def _split(data):
    """(the four correspondence tensors, the weights as one tensor over the records -- ones where absent)"""
    d = {k: v for k, v in data.items() if k in NAMES[:4] and v is not None and len(v)}
    n_p = len(d["pts_3d"]) if "pts_3d" in d else 0
    n_l = len(d["line_3d"]) if "line_3d" in d else 0
    wp, wl = data.get("weights_pts"), data.get("weights_lines")
    parts = []
    if n_p:
        parts.append(torch.ones(n_p, dtype=F64) if wp is None else wp)
    if n_l:
        parts.append(torch.ones(n_l, dtype=F64) if wl is None else wl)
    return d, torch.cat(parts)


def _system(R, t, K, d, w, c, loss, delta, variant="full", rows=False):
    """s, g, H (and the rows J of the residuals' Jacobian, the residuals) at xi = 0 of the chart about c, the graph of g kept."""
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    R1, t1 = pose_of(xi, R, t, c)
    r = residuals(R1, t1, K, **d)
    s = (r * r).sum(1)
    if variant == "full":
        F = 0.5 * (w * rho(loss, s, delta)).sum()
    else:  # rho' a constant of the pose and of the data
        s0 = s.detach().clone().requires_grad_(True)
        (rp,) = torch.autograd.grad(rho(loss, s0, delta).sum(), s0)
        F = 0.5 * (w * rp * s).sum()
    (g,) = torch.autograd.grad(F, xi, create_graph=True)
    H = torch.stack([torch.autograd.grad(g[i], xi, retain_graph=True)[0] for i in range(6)])
    H = 0.5 * (H + H.T)
    J = None
    if rows:
        rf = r.reshape(-1)
        J = torch.stack([torch.autograd.grad(rf[k], xi, retain_graph=True)[0] for k in range(len(rf))])
    return s.detach(), g, H, J, r.detach()


def squares(R, t, K, **data):
    """s_k of every record at a pose (numpy)."""
    d, _ = _split({k: _t(v) for k, v in data.items() if v is not None})
    r = residuals(_t(R), _t(t), _t(K), **d)
    return (r * r).sum(1).numpy()


def stationarity(R, t, K, loss, delta, c=None, **data):
    """(|g| / sum_k omega_k sum_i |J_i| |r_i|, rms residual, smallest eigenvalue of the full H over its largest, the ratio's
    representability floor eps |t| |H| / scale: tests/refine_grad_reference.py) of a pose, in the chart about c (default: the centre)."""
    d, w = _split({k: _t(v) for k, v in data.items() if v is not None})
    c = _t(centre_of(d.get("pts_3d"), d.get("line_3d")) if c is None else c)
    s, g, H, J, r = _system(_t(R), _t(t), _t(K), d, w, c, loss, delta, rows=True)
    s0 = s.clone().requires_grad_(True)
    (rp,) = torch.autograd.grad(rho(loss, s0, delta).sum(), s0)
    om = (w * rp).repeat_interleave(2)
    ev = torch.linalg.eigvalsh(H.detach())
    scale = float((om * J.norm(dim=1) * r.reshape(-1).abs()).sum()) + 1e-300
    floor = float(np.finfo(np.float64).eps * np.linalg.norm(t) * ev.abs().max()) / scale
    return float(g.detach().norm()) / scale, float(r.pow(2).mean().sqrt()), float(ev[0] / ev[-1]), floor


def _cost(R, t, K, d, w, loss, delta):
    r = residuals(R, t, K, **d)
    return float(0.5 * (w * rho(loss, (r * r).sum(1), delta)).sum())


def polish(R, t, K, loss, delta, iters=40, tol=1e-28, pure=False, descend=True, **data):
    """The minimiser of F near (R, t), as numpy arrays (R, t), in the centred chart.  First a descent that cannot leave the basin: steps
    of the Hessian without the rho'' term (positive definite), halved until F falls, until they are short.  Then Newton's method with
    the full Hessian; the pose with the smallest |g| is returned, and the run ends when |g|^2 <= tol or |g| has stopped falling (the
    rounding floor of the scene).  pure: Newton's method alone with its step halved until |g| falls, which also converges to stationary
    points that are not minima.  descend=False: no descent, for a start that is already next to the minimiser."""
    d, w = _split({k: _t(v) for k, v in data.items() if v is not None})
    c = _t(centre_of(d.get("pts_3d"), d.get("line_3d")))
    R, t, K = _t(R), _t(t), _t(K)
    for _ in range(60 if descend and not pure else 0):
        _, g, H, _, _ = _system(R, t, K, d, w, c, loss, delta, variant="struck")
        step, f0 = -torch.linalg.solve(H.detach(), g.detach()), _cost(R, t, K, d, w, loss, delta)
        for _ in range(30):
            R1, t1 = (x.detach() for x in pose_of(step, R, t, c))
            if _cost(R1, t1, K, d, w, loss, delta) <= f0:
                break
            step = 0.5 * step
        else:
            break
        R, t = R1, t1
        if float(step.norm()) <= 1e-7:
            break
    best, stalls = None, 0
    for _ in range(iters):
        _, g, H, _, _ = _system(R, t, K, d, w, c, loss, delta)
        g, H = g.detach(), H.detach()
        gn = float(g.norm())
        if best is None or gn < best[0]:
            best, stalls = (gn, R, t), 0
        else:
            stalls += 1
        if gn * gn <= tol or stalls >= 2:
            break
        step = -torch.linalg.solve(H, g)
        for _ in range(20 if pure else 0):   # (a saddle has no cost to descend on: the step is halved until |g| falls)
            R1, t1 = (x.detach() for x in pose_of(step, R, t, c))
            if float(_system(R1, t1, K, d, w, c, loss, delta)[1].detach().norm()) < gn:
                break
            step = 0.5 * step
        R, t = (x.detach() for x in pose_of(step, R, t, c))
    _, R, t = best
    return R.numpy().copy(), t.numpy().copy()


def reference_vjp(R, t, K, loss, delta, grad_R=None, grad_t=None, centred=True, variant="full", **data):
    """dict of dL/d(pts_2d, pts_3d, line_2d, line_3d, weights_pts, weights_lines) (numpy, None where the kind is absent; the weights'
    gradients also where the weights are: the derivative at w = 1) of ONE problem at the pose (R, t), plus "H", "g" and "psi"."""
    n_p = len(data["pts_3d"]) if data.get("pts_3d") is not None else 0
    n_l = len(data["line_3d"]) if data.get("line_3d") is not None else 0
    data = dict(data)
    if n_p and data.get("weights_pts") is None:
        data["weights_pts"] = np.ones(n_p)
    if n_l and data.get("weights_lines") is None:
        data["weights_lines"] = np.ones(n_l)
    leaves = {k: _t(v).clone().requires_grad_(True) for k, v in data.items() if v is not None and len(v)}
    d, w = _split(leaves)
    c = _t(centre_of(data.get("pts_3d"), data.get("line_3d"))) if centred else torch.zeros(3, dtype=F64)
    R, t, K = _t(R), _t(t), _t(K)
    GR = torch.zeros(3, 3, dtype=F64) if grad_R is None else _t(grad_R)
    gt = torch.zeros(3, dtype=F64) if grad_t is None else _t(grad_t)
    _, g, H, _, _ = _system(R, t, K, d, w, c, loss, delta, variant)
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    R1, t1 = pose_of(xi, R, t, c)
    (b,) = torch.autograd.grad((GR * R1).sum() + (gt * t1).sum(), xi)
    psi = torch.linalg.solve(H.detach(), b)
    keys = list(leaves)
    grads = torch.autograd.grad(-(g * psi).sum(), [leaves[k] for k in keys], allow_unused=True)
    out = {k: None for k in NAMES}
    for k, v in zip(keys, grads):
        out[k] = (torch.zeros_like(leaves[k]) if v is None else v).numpy().copy()
    out.update(H=H.detach().numpy().copy(), g=g.detach().numpy().copy(), psi=psi.numpy().copy())
    return out


def flat(out, b=None, names=NAMES):
    """The gradients as one vector (problem b of a batch result, or a single-problem dict)."""
    parts = []
    for k in names:
        v = out.get(k)
        if v is not None:
            parts.append(np.asarray(v if b is None else v[b]).reshape(-1))
    return np.concatenate(parts)


def rel_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def truth_and_floor(R, t, K, loss, delta, grad_R, grad_t, **data):
    """(the centred reference's gradients as one vector, its disagreement with the plain chart: the reference's own floor)."""
    a = flat(reference_vjp(R, t, K, loss, delta, grad_R, grad_t, centred=True, **data))
    b = flat(reference_vjp(R, t, K, loss, delta, grad_R, grad_t, centred=False, **data))
    return a, rel_err(b, a)


def minimiser_value(R, t, K, loss, delta, grad_R, grad_t, **data):
    """<G_R, R*> + <g_t, t*> at the reference's own minimiser of the data, by Newton's method from (R, t), a pose next to it."""
    R1, t1 = polish(R, t, K, loss, delta, iters=8, descend=False, **data)
    return float((np.asarray(grad_R) * R1).sum() + (np.asarray(grad_t) * t1).sum())
