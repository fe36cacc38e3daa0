"""The DEFINITION of the gradient of a refined pose, in torch float64 autograd on the CPU -- what tests/test_refine_grad_host.py holds
cvxpnpl_refine_vjp_batch_host (csrc/refine_vjp_core.h, the source of the kernels) against.  Nothing is imported from cvxpnpl_amd and no
formula of the core is restated: the residuals are written from the definition of DESIGN.md section 15 with torch.matrix_exp,

    Y = R X + t,  (u, v) = pi(K Y);  a point gives (u - x, v - y);  a line (a, b) <-> (E0, E1) gives l . (u_k, v_k, 1) for both end points,
    l = (a, 1) x (b, 1) / hypot(l_0, l_1),

the cost is f = 1/2 sum rho^2, its gradient g and Hessian H in the chart xi = (w, tau) come from double backward, the upstream covector b
is the gradient at xi = 0 of <G_R, R(xi)> + <g_t, t(xi)>, and

    dL/dtheta = -(dg/dtheta)^T H^-1 b = -d/dtheta (g . psi),  psi = H^-1 b held fixed.

Two charts: the plain one, R' = exp([w]x) R, t' = t + tau, and the one centred on a point c, X -> exp([w]x) R (X - c) + R c + t + tau.  At a
stationary pose both give the same gradients; the centred one is the truth (well conditioned for scenes far from the origin), and their
disagreement is the reference's own noise floor.  hessian="gn" swaps in the Gauss-Newton matrix J^T J: the shortcut the tests must tell
apart.  The module carries a Newton polish of its own (full Hessian, centred chart)."""
import numpy as np
import torch

F64 = torch.float64
NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d")


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
    """All residuals of a pose, points first (u - x, v - y per point), then both end points of every line."""
    out = []

    def pix(X):
        h = (X @ R.T + t) @ K.T
        return h[..., :2] / h[..., 2:]

    if pts_3d is not None and len(pts_3d):
        out.append((pix(pts_3d) - pts_2d).reshape(-1))
    if line_3d is not None and len(line_3d):
        a, b = line_2d[:, 0], line_2d[:, 1]
        one = torch.ones(len(a), 1, dtype=F64)
        l = torch.linalg.cross(torch.cat([a, one], 1), torch.cat([b, one], 1))
        l = l / torch.hypot(l[:, 0], l[:, 1])[:, None]
        uv = pix(line_3d)                                            # [n, 2, 2]
        out.append((l[:, None, 0] * uv[..., 0] + l[:, None, 1] * uv[..., 1] + l[:, None, 2]).reshape(-1))
    return torch.cat(out)


def centre_of(pts_3d=None, line_3d=None):
    rows = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pts_3d, line_3d) if x is not None and len(x)]
    return np.concatenate(rows).mean(0)


def _system(R, t, K, data, c, hessian="full"):
    """rho, J, g, H at xi = 0 of the chart about c, with the graph of g kept (for the derivative with respect to the data)."""
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    R1, t1 = pose_of(xi, R, t, c)
    rho = residuals(R1, t1, K, **data)
    f = 0.5 * (rho * rho).sum()
    (g,) = torch.autograd.grad(f, xi, create_graph=True)
    J = torch.stack([torch.autograd.grad(rho[k], xi, retain_graph=True)[0] for k in range(len(rho))])
    if hessian == "gn":
        H = J.T @ J
    else:
        H = torch.stack([torch.autograd.grad(g[i], xi, retain_graph=True)[0] for i in range(6)])
        H = 0.5 * (H + H.T)
    return rho.detach(), J, g, H, xi


def stationarity(R, t, K, c=None, **data):
    """(|g| / sum_k |J_k| |rho_k|, rms rho, smallest eigenvalue of the full H over its largest, the ratio's representability floor) of a
    pose, in the chart about c (default: the centre of the 3D records).  The floor: t is stored to eps |t|, which alone moves g by up to
    eps |t| |H| -- for a scene 1e4 from the origin more than 1e-12 of the scale, whatever polished the pose."""
    d = {k: _t(v) for k, v in data.items() if v is not None}
    c = _t(centre_of(d.get("pts_3d"), d.get("line_3d")) if c is None else c)
    rho, J, g, H, _ = _system(_t(R), _t(t), _t(K), d, c)
    ev = torch.linalg.eigvalsh(H)
    scale = float((J.norm(dim=1) * rho.abs()).sum()) + 1e-300
    floor = float(np.finfo(np.float64).eps * np.linalg.norm(t) * ev.abs().max()) / scale
    return float(g.detach().norm()) / scale, float(rho.pow(2).mean().sqrt()), float(ev[0] / ev[-1]), floor


def polish(R, t, K, iters=30, tol=1e-13, **data):
    """Newton's method on f with the full Hessian in the centred chart, from (R, t): returns (R, t) as numpy arrays.  Stops when
    |g| <= tol sum |J||rho| or when the residuals are at rounding level (an exact fit)."""
    d = {k: _t(v) for k, v in data.items() if v is not None}
    c = _t(centre_of(d.get("pts_3d"), d.get("line_3d")))
    R, t, K = _t(R), _t(t), _t(K)
    best = None
    for _ in range(iters):
        rho, J, g, H, _ = _system(R, t, K, d, c)
        g = g.detach()
        rel = float(g.norm() / ((J.norm(dim=1) * rho.abs()).sum() + 1e-300))
        if best is None or float(g.norm()) < best[0]:   # (|g| itself: at an exact fit the ratio is rounding noise)
            best = (float(g.norm()), R, t)
        if rel <= tol or float(rho.pow(2).mean().sqrt()) <= 1e-12:
            break
        if best[0] < float(g.norm()) and len(rho) > 6:   # |g| has stopped falling: the rounding floor of this scene
            break
        step = -torch.linalg.solve(H, g)
        R, t = (x.detach() for x in pose_of(step, R, t, c))
    _, R, t = best
    return R.numpy().copy(), t.numpy().copy()


def reference_vjp(R, t, K, grad_R=None, grad_t=None, centred=True, hessian="full", **data):
    """dict of dL/d(pts_2d, pts_3d, line_2d, line_3d) (numpy, None where absent) of ONE problem at the pose (R, t), plus "H", "g" and
    "psi".  centred: chart about the centre of the 3D records (the truth); otherwise the plain chart."""
    d = {k: _t(v).clone().requires_grad_(True) for k, v in data.items() if v is not None and len(v)}
    c = _t(centre_of(data.get("pts_3d"), data.get("line_3d"))) if centred else torch.zeros(3, dtype=F64)
    R, t, K = _t(R), _t(t), _t(K)
    GR = torch.zeros(3, 3, dtype=F64) if grad_R is None else _t(grad_R)
    gt = torch.zeros(3, dtype=F64) if grad_t is None else _t(grad_t)
    _, _, g, H, _ = _system(R, t, K, d, c, hessian)
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    R1, t1 = pose_of(xi, R, t, c)
    (b,) = torch.autograd.grad((GR * R1).sum() + (gt * t1).sum(), xi)
    psi = torch.linalg.solve(H.detach(), b)
    keys = list(d)
    grads = torch.autograd.grad(-(g * psi).sum(), [d[k] for k in keys], allow_unused=True)
    out = {k: None for k in NAMES}
    for k, v in zip(keys, grads):
        out[k] = (torch.zeros_like(d[k]) if v is None else v).numpy().copy()
    out.update(H=H.detach().numpy().copy(), g=g.detach().numpy().copy(), psi=psi.numpy().copy())
    return out


def flat(out, b=None):
    """The four gradients as one vector (problem b of a batch result, or a single-problem dict)."""
    parts = []
    for k in NAMES:
        v = out.get(k)
        if v is not None:
            parts.append(np.asarray(v if b is None else v[b]).reshape(-1))
    return np.concatenate(parts)


def rel_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def truth_and_floor(R, t, K, grad_R, grad_t, **data):
    """(the centred reference's gradients as one vector, its disagreement with the plain chart: the reference's own floor)."""
    a = flat(reference_vjp(R, t, K, grad_R, grad_t, centred=True, **data))
    b = flat(reference_vjp(R, t, K, grad_R, grad_t, centred=False, **data))
    return a, rel_err(b, a)
