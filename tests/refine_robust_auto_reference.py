"""Independent reference of the scale estimate and the sandwich covariance (cvxpnpl_amd/csrc/refine_robust_auto_core.h), numpy only, no
library code.

``sigma_hat``: s_k of the live records from tests/refine_robust_reference.py's ``squares``, numpy.median, sqrt(median / (2 ln 2)).

``sandwich``: the covariance  m / (m - 6) H^-1 B H^-1  from central differences in long double of RHO ITSELF -- never rho' or rho'' -- in
the public chart xi = (w, tau), R' = exp([w]x) R, t' = t + tau:
  g_k = the gradient of  1/2 w_k rho(s_k(xi))  at xi = 0, one per live record;      B = sum_k g_k g_k^T;
  H   = the difference Jacobian of  xi -> sum_k g_k(xi)  at xi = 0 (symmetrised).
Both differences are the sixth-order stencil with step h, so every evaluation lies within 3 h (6 h for H) of the pose.  Under Huber h is
small -- 1e-7 -- because that loss is only once differentiable: no record may cross s = delta^2 inside the stencil
(tests/refine_robust_auto_cases.py asserts the margin); l2 and Cauchy are smooth and take 1e-5.  What a step costs in rounding is measured,
not assumed: ``sandwich`` returns its own FLOOR, the disagreement
between the result at h and at h / 2 relative to |V|_F.
"""
import numpy as np

import refine_reference as ref
import refine_robust_reference as rr

CHI2_2_MEDIAN = 1.3862943611198906  # 2 ln 2
H_STEP = {"huber": 1e-7, "l2": 1e-5, "cauchy": 1e-5}
_C = ((1, 45.0), (2, -9.0), (3, 1.0))  # f'(0) ~ sum_a c_a (f(a h) - f(-a h)) / (60 h)


def sigma_hat(K, R, t, **data):
    """(sigma, med_sq, s of the live records, points then lines)"""
    s = rr.squares(K, R, t, **data)[0]
    med = float(np.median(s))
    return float(np.sqrt(med / CHI2_2_MEDIAN)), med, s


def entry_status(K, R, t, **data):
    """The refinement's entry checks in its order (rr.refine's): 2, 4 (a bad weight), 3, 4 (behind the camera or non-finite), else 0."""
    R, t = np.asarray(R, float), np.asarray(t, float)
    lp, ll, _, _, bad = rr.live_weights(**data)
    if not np.all(np.isfinite(R)) or not np.all(np.isfinite(t)) or not np.linalg.det(R) > 0:
        return 2
    if bad:
        return 4
    if int(lp.sum() + ll.sum()) < 3:
        return 3
    with np.errstate(invalid="ignore", over="ignore"):
        s, _, _, _, zmin = rr.squares(K, R, t, **data)
    if not np.all(np.isfinite(s)) or not zmin > 0:
        return 4
    return 0


def _half_costs(Kl, Rl, tl, loss, delta, dl, xi):
    """1/2 w_k rho(s_k) of every live record at the pose moved by xi, long double"""
    s, w, _, _, _ = rr.squares(Kl, ref.expm_so3(xi[:3]) @ Rl, tl + xi[3:], **dl)
    return 0.5 * w * rr.rho(loss, s, np.longdouble(delta))


def _grads(f, xi0, h):
    """[6, n]: the gradient of every component of f at xi0"""
    ld = np.longdouble
    out = []
    for k in range(6):
        acc = 0
        for a, c in _C:
            e = np.zeros(6, ld)
            e[k] = a * h
            acc = acc + c * (f(xi0 + e) - f(xi0 - e))
        out.append(acc / (60 * ld(h)))
    return np.stack(out)


def _sandwich_at(K, R, t, loss, delta, h, data):
    ld = np.longdouble
    Kl, Rl, tl = np.asarray(K, ld), np.asarray(R, ld), np.asarray(t, ld)
    dl = {k: (np.asarray(v, ld) if v is not None and not k.startswith("mask") else v) for k, v in data.items()}

    def f(xi):
        return _half_costs(Kl, Rl, tl, loss, delta, dl, xi)

    G = _grads(f, np.zeros(6, ld), h)               # [6, n]
    B = G @ G.T

    def gsum(xi):
        return _grads(f, xi, h).sum(1)              # [6]

    H = _grads(gsum, np.zeros(6, ld), h)            # [6, 6]: row k is d gsum / d xi_k
    H = 0.5 * (H + H.T)
    n = G.shape[1]
    m = 2 * n
    Hi = np.linalg.inv(H.astype(np.float64))
    # one step of refinement of the inverse in long double, so that the solve does not set the floor
    Hi = Hi.astype(ld)
    Hi = Hi + Hi @ (np.eye(6, dtype=ld) - H @ Hi)
    V = (ld(m) / ld(m - 6)) * (Hi @ B @ Hi)
    return V.astype(np.float64), H.astype(np.float64), B.astype(np.float64)


def sandwich(K, R, t, loss, delta, h=None, **data):
    """(V [6,6] in the public chart, floor, H, B): floor = |V(h) - V(h / 2)|_F / |V(h)|_F; h: H_STEP of the loss"""
    h = H_STEP[loss] if h is None else h
    V, H, B = _sandwich_at(K, R, t, loss, delta, h, data)
    V2, _, _ = _sandwich_at(K, R, t, loss, delta, 0.5 * h, data)
    return V, float(np.linalg.norm(V - V2) / np.linalg.norm(V)), H, B


def hessian_and_meat(K, R, t, loss, delta, h=None, **data):
    """(H, B, floor of H, floor of B) in the public chart: the two halves of ``sandwich`` on their own, each with the disagreement between
    the steps h and h / 2 relative to its Frobenius norm"""
    h = H_STEP[loss] if h is None else h
    _, H, B = _sandwich_at(K, R, t, loss, delta, h, data)
    _, H2, B2 = _sandwich_at(K, R, t, loss, delta, 0.5 * h, data)
    return H, B, float(np.linalg.norm(H - H2) / np.linalg.norm(H)), float(np.linalg.norm(B - B2) / np.linalg.norm(B))
