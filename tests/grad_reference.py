"""An independent reference for the pose VJP, and the helpers the gradient tests share -- a plain module, not a test file.

``reference_vjp`` is the *definition* in torch float64 autograd on the CPU: the algebraic cost
    f = sum_points |[K^-1 x~]x (R X + t)|^2 + sum_lines sum_ends (n . (R L + t))^2,   n = (a x b) / |a x b|,
a chart xi = (w, tau) of the pose that rotates about ``centre`` (R(xi) = exp([w]x) R0, t(xi) = R0 c + t0 + tau - R(xi) c),
g = df/dxi, H = dg/dxi and b = d(<G_R, R> + <g_t, t>)/dxi by autograd (H and dg/dtheta by double backward), and
dL/dtheta = -(dg/dtheta)^T H^-1 b.  It shares nothing with cvxpnpl_amd (no import, no formula of vjp_core.h: torch.matrix_exp,
torch.cross and autograd only), nothing in it assumes det R = +1, and it runs wherever torch runs.

Its own noise floor: at a stationary pose every chart gives the same gradients, so the reference with centre = mean of the 3D
records (the truth: H is well conditioned there) and with centre = 0 (the plain chart, whose rotation-translation coupling grows
with |centre|^2) must agree; ``reference_floor`` returns their disagreement.

``polish`` makes a pose stationary to rounding without the oracle (Gauss-Newton of the test's own; only g = 0 matters).
"""
import numpy as np
import torch

NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d")


# ------------------------------------------------------------------------------------------------ the polished solve (numpy)
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _expm(w):
    th = np.linalg.norm(w)
    W = _hat(w)
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th ** 2 * W @ W


def _rows(R, t, p2, p3, l2, l3, Ki):
    """Residual rows A_i (R X_i + t) as (A [m,3], X [m,3])."""
    A, X = [], []
    for uv, P in zip(p2, p3):
        p = Ki @ np.array([uv[0], uv[1], 1.0])
        A.append(_hat(p))
        X.append(np.repeat(P[None], 3, 0))
    for seg, ends in zip(l2, l3):
        a = Ki @ np.array([seg[0, 0], seg[0, 1], 1.0])
        b = Ki @ np.array([seg[1, 0], seg[1, 1], 1.0])
        n = np.cross(a, b)
        n /= np.linalg.norm(n)
        for E in ends:
            A.append(n[None])
            X.append(E[None])
    return np.concatenate(A), np.concatenate(X)


def polish(R, t, p2, p3, l2, l3, K, iters=60):
    """Gauss-Newton on the algebraic cost about the centroid c of the 3D records (X -> exp(w) R (X - c) + tc + tau) until the step is
    at rounding level.  Returns R, t and the final |g| relative to its Cauchy-Schwarz bound."""
    Ki = np.linalg.inv(K)
    A, X = _rows(R, t, p2, p3, l2, l3, Ki)
    c = X.mean(0)
    tc = R @ c + t
    for _ in range(iters):
        y = (X - c) @ R.T
        z = y + tc
        r = np.einsum("ij,ij->i", A, z)
        J = np.concatenate([np.cross(y, A), A], 1)  # d/dw of a.(exp(w) y) = a.(w x y) = w.(y x a)
        g = 2 * J.T @ r
        step = -np.linalg.solve(J.T @ J, J.T @ r)
        R = _expm(step[:3]) @ R
        tc = tc + step[3:]
        if np.abs(step).max() < 1e-17 * (1 + np.abs(tc).max()):
            break
    t = tc - R @ c
    return R, t, np.linalg.norm(g) / (2 * np.sqrt((J ** 2).sum() * (r @ r)) + 1e-300)


def exact_fit(R, t, p2, p3, l2, l3, K):
    """|r| / sqrt(sum |A_i|^2 |z_i|^2): the residual relative to the size of its terms.  At rounding level (noise-free data, or a
    minimal problem that the pose fits exactly) g = 2 J^T r vanishes with r, and polish's ratio |g| / (2 |J| |r|) is 0 / 0."""
    A, X = _rows(R, t, p2, p3, l2, l3, np.linalg.inv(K))
    z = X @ R.T + t
    return np.linalg.norm(np.einsum("ij,ij->i", A, z)) / np.sqrt(((A ** 2).sum(1) * (z ** 2).sum(1)).sum())


# ------------------------------------------------------------------------------------------------ the reference (torch autograd)
def _t64(x, shape):
    return torch.as_tensor(np.asarray(x, dtype=np.float64).reshape(shape), dtype=torch.float64).clone()


def _skew(w):
    o = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([o, -w[2], w[1]]), torch.stack([w[2], o, -w[0]]), torch.stack([-w[1], w[0], o])])


def _cost(R, t, p2, p3, l2, l3, Ki):
    f = torch.zeros((), dtype=torch.float64)
    if p3.shape[0]:
        p = torch.cat([p2, torch.ones_like(p2[:, :1])], 1) @ Ki.T
        f = f + (torch.cross(p, p3 @ R.T + t, dim=1) ** 2).sum()
    if l3.shape[0]:
        ab = torch.cat([l2, torch.ones_like(l2[..., :1])], 2) @ Ki.T  # [n,2,3]
        m = torch.cross(ab[:, 0], ab[:, 1], dim=1)
        n = m / m.norm(dim=1, keepdim=True)
        f = f + ((((l3 @ R.T) + t) * n[:, None, :]).sum(2) ** 2).sum()
    return f


def reference_vjp(R, t, pts_2d, pts_3d, line_2d, line_3d, K, G_R, g_t, centre):
    """dL/d(pts_2d, pts_3d, line_2d, line_3d) of one problem at the stationary pose (R, t) (R in O(3)), for the upstream dL/dR = G_R,
    dL/dt = g_t, in the chart that rotates about ``centre``.  Arrays in, a dict of numpy arrays out (None for an absent kind)."""
    R0, t0, c = _t64(R, (3, 3)), _t64(t, (3,)), _t64(centre, (3,))
    Ki = torch.linalg.inv(_t64(K, (3, 3)))
    G, gt = _t64(G_R, (3, 3)), _t64(g_t, (3,))
    n_p = 0 if pts_3d is None else int(np.asarray(pts_3d).size // 3)
    n_l = 0 if line_3d is None else int(np.asarray(line_3d).size // 6)
    theta = {"pts_2d": _t64(pts_2d if n_p else np.zeros(0), (n_p, 2)), "pts_3d": _t64(pts_3d if n_p else np.zeros(0), (n_p, 3)),
             "line_2d": _t64(line_2d if n_l else np.zeros(0), (n_l, 2, 2)), "line_3d": _t64(line_3d if n_l else np.zeros(0), (n_l, 2, 3))}
    leaves = [theta[k].requires_grad_() for k in NAMES]
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)

    def pose(xi):
        Rx = torch.matrix_exp(_skew(xi[:3])) @ R0
        return Rx, R0 @ c + t0 + xi[3:] - Rx @ c

    Rx, tx = pose(xi)
    f = _cost(Rx, tx, theta["pts_2d"], theta["pts_3d"], theta["line_2d"], theta["line_3d"], Ki)
    (g,) = torch.autograd.grad(f, xi, create_graph=True)
    H = torch.stack([torch.autograd.grad(g[i], xi, retain_graph=True)[0] for i in range(6)])
    Rb, tb = pose(xi)
    (b,) = torch.autograd.grad((G * Rb).sum() + (gt * tb).sum(), xi)
    v = torch.linalg.solve(0.5 * (H + H.T), b)
    grads = torch.autograd.grad(-(g * v).sum(), leaves, allow_unused=True)
    return {k: (None if theta[k].numel() == 0 else (torch.zeros_like(theta[k]) if gr is None else gr).numpy()) for k, gr in zip(NAMES, grads)}


def records(pts_3d, line_3d):
    """The 3D records of one problem ([m,3]: points, then line end points)."""
    parts = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pts_3d, line_3d) if x is not None and np.asarray(x).size]
    return np.concatenate(parts)


def flat(out, b=None):
    """The four gradients of a result dict (of problem b, if given) as one vector."""
    return np.concatenate([np.asarray(out[k] if b is None else out[k][b], dtype=np.float64).ravel() for k in NAMES if out.get(k) is not None])


def rel_err(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def reference_truth_and_floor(R, t, p2, p3, l2, l3, K, G_R, g_t):
    """The centred-chart reference (the truth) as one vector, and its relative disagreement with the plain chart (the floor)."""
    truth = flat(reference_vjp(R, t, p2, p3, l2, l3, K, G_R, g_t, records(p3, l3).mean(0)))
    plain = flat(reference_vjp(R, t, p2, p3, l2, l3, K, G_R, g_t, np.zeros(3)))
    return truth, rel_err(plain, truth)


# ------------------------------------------------------------------------------------------------ scenes
def per_problem_K(d, seed):
    """A camera per problem (focal length and skew vary); the pixels of d re-projected through it with the noise drawn again (1 px)."""
    batch = d["pts_3d"].shape[0]
    n_p, n_l = d["pts_3d"].shape[1], d["line_3d"].shape[1]
    Kin = np.repeat(np.asarray(d["K"], dtype=np.float64)[None], batch, 0)
    Kin[:, 0, 0] *= 1.0 + 0.3 * np.linspace(-1, 1, batch)
    Kin[:, 0, 1] = 2.0 * np.linspace(-1, 1, batch) + 0.5
    rs = np.random.RandomState(seed)
    for key, P, shp in (("pts_2d", d["pts_3d"], (batch, n_p, 2)), ("line_2d", d["line_3d"], (batch, n_l, 2, 2))):
        P = P.reshape(batch, -1, 3)
        h = np.einsum("bij,bnj->bni", Kin, np.einsum("bij,bnj->bni", d["R_gt"], P) + d["t_gt"][:, None])
        d[key] = np.ascontiguousarray((h[..., :2] / h[..., 2:] + rs.normal(size=h[..., :2].shape)).reshape(shp))
    d["K"] = Kin
    return d


def problem(d, b):
    """(p2, p3, l2, l3, K) of problem b, absent kinds as empty arrays."""
    K = d["K"][b] if d["K"].ndim == 3 else d["K"]
    return d["pts_2d"][b], d["pts_3d"][b], d["line_2d"][b], d["line_3d"][b], K


def polish_batch(d, idx=None):
    """Polished poses of the problems idx of d (all by default), started at the ground truth: R [m,3,3], t [m,3], |g|_rel [m] and
    the exact-fit ratio [m]."""
    idx = range(d["pts_3d"].shape[0]) if idx is None else idx
    Rs, ts, gs, fits = [], [], [], []
    for b in idx:
        R, t, g = polish(d["R_gt"][b], d["t_gt"][b], *problem(d, b))
        Rs.append(R), ts.append(t), gs.append(g), fits.append(exact_fit(R, t, *problem(d, b)))
    return np.stack(Rs), np.stack(ts), np.array(gs), np.array(fits)


def kinds(d):
    """The keyword arguments of pose_vjp / pose_vjp_host for the correspondences of d (None for an absent kind)."""
    n_p, n_l = d["pts_3d"].shape[1], d["line_3d"].shape[1]
    return dict(pts_2d=d["pts_2d"] if n_p else None, pts_3d=d["pts_3d"] if n_p else None,
                line_2d=d["line_2d"] if n_l else None, line_3d=d["line_3d"] if n_l else None)
