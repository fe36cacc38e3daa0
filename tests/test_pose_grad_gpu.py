"""The pose VJP on the device (cvxpnpl_pose_vjp_batch) and the autograd path (-m gpu).

The device kernels and the host loop (cvxpnpl_pose_vjp_host, checked against finite differences in test_pose_grad_host.py) are one
source (vjp_core.h); only the order of the sums differs, so they agree to 1e-10 relative at the GPU's own poses -- in both regimes
(16 lanes per problem; the multi-workgroup reduction from 768 records on).  Every status here comes from a real solve, where nearly
all problems certify: the skipped, singular and non-finite problems of either regime, the regime boundary, the workgroup tails, absent
arguments, side streams and the comparison with an independent reference are in test_pose_grad_gpu_edges.py (the reference itself
in grad_reference.py, the host twin against it in test_pose_grad_reference.py).
"""
import numpy as np
import pytest
import torch

from cvxpnpl_amd import pnpl_batch, synth
from cvxpnpl_amd.grad import ADMIT_CERTIFIED, ADMIT_RANK1, pnl_batch_diff, pnp_batch_diff, pnpl_batch_diff, pose_vjp, pose_vjp_host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("pts_2d", "pts_3d", "line_2d", "line_3d")


def _t(x):
    return torch.as_tensor(x, device=DEV) if x is not None else None


def _compare(batch, n_p, n_l, seed, K=synth.K_KINECT, K_per_problem=False, admit=ADMIT_CERTIFIED, info=False):
    d = synth.make_pnpl(batch, n_p, n_l, sigma=1.0 if not K_per_problem else 0.0, seed=seed, K=K)
    Kin = d["K"]
    if K_per_problem:  # a camera per problem (focal lengths and skew vary), pixels re-projected through it with 1 px noise
        Kin = np.repeat(d["K"][None], batch, 0)
        Kin[:, 0, 0] *= 1.0 + 0.3 * np.linspace(-1, 1, batch)
        Kin[:, 0, 1] = 2.0 * np.linspace(-1, 1, batch)
        rs = np.random.RandomState(seed)
        for key, P, shp in (("pts_2d", d["pts_3d"], (batch, n_p, 2)), ("line_2d", d["line_3d"], (batch, n_l, 2, 2))):
            P = P.reshape(batch, -1, 3)
            h = np.einsum("bij,bnj->bni", Kin, np.einsum("bij,bnj->bni", d["R_gt"], P) + d["t_gt"][:, None])
            d[key] = np.ascontiguousarray((h[..., :2] / h[..., 2:] + rs.normal(size=h[..., :2].shape)).reshape(shp))
    args = dict(pts_2d=d["pts_2d"] if n_p else None, line_2d=d["line_2d"] if n_l else None, pts_3d=d["pts_3d"] if n_p else None,
                line_3d=d["line_3d"] if n_l else None)
    res = pnpl_batch(*(_t(args[k]) for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")), _t(Kin))
    rng = np.random.default_rng(seed)
    gR, gt = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
    dev = pose_vjp(res.R, res.t, res.status, _t(gR), _t(gt), K=_t(Kin), admit_mask=admit, want_info=info, **{k: _t(v) for k, v in args.items()})
    torch.cuda.synchronize()
    R, t, st = res.R.cpu().numpy(), res.t.cpu().numpy(), res.status.cpu().numpy()
    host = pose_vjp_host(R, t, st, gR, gt, K=Kin, admit_mask=admit, **args)
    vst = dev["vjp_status"].cpu().numpy()
    assert (vst == host["vjp_status"]).all()
    assert (vst == 0).mean() > 0.9, np.bincount(vst)
    num = np.zeros(batch)
    den = np.zeros(batch)
    for name in NAMES:
        if dev[name] is None:
            continue
        a, b = dev[name].cpu().numpy().reshape(batch, -1), host[name].reshape(batch, -1)
        assert np.isfinite(a).all()
        assert not a[vst != 0].any()
        num += ((a - b) ** 2).sum(1)
        den += (b ** 2).sum(1)
    ok = vst == 0
    rel = np.sqrt(num[ok] / den[ok])
    assert rel.max() < 1e-10, (rel.max(), np.argmax(rel))
    if info:
        di = dev["info"].cpu().numpy()
        assert np.allclose(di[ok, 0], host["info"][ok, 0], rtol=1e-6)  # lambda_min / lambda_max
        assert np.allclose(di[ok, 1], host["info"][ok, 1], rtol=1e-3, atol=1e-11)  # |g|: the same up to the rounding of the sums
    return rel.max()


@pytest.mark.parametrize("batch,n_p,n_l,K_per,info", [(10_000, 10, 0, False, False), (4096, 4, 0, False, True), (2000, 0, 6, False, False),
                                                      (2000, 5, 5, False, True), (1000, 10, 0, True, False), (1000, 5, 5, True, False)],
                         ids=["pnp10-10k", "pnp4", "pnl6", "pnpl5+5", "pnp10-Kper", "pnpl5+5-Kper"])
def test_device_matches_host_small_n(batch, n_p, n_l, K_per, info):
    _compare(batch, n_p, n_l, seed=batch + n_p + n_l, K_per_problem=K_per, info=info)


@pytest.mark.parametrize("batch,n_p,n_l,info", [(5, 10_000, 0, True), (64, 2000, 0, False), (8, 600, 300, True)],
                         ids=["5x1e4", "64x2000", "pnpl-600+300"])
def test_device_matches_host_large_n(batch, n_p, n_l, info):
    _compare(batch, n_p, n_l, seed=7 + batch, info=info)


def test_rank1_admission_on_device():
    _compare(2000, 4, 0, seed=99, admit=ADMIT_RANK1)


def test_autograd_matches_pose_vjp_and_leaves_the_rest_none():
    d = synth.make_pnpl(512, 6, 4, sigma=1.0, seed=5)
    p2 = _t(d["pts_2d"]).requires_grad_()
    l2 = _t(d["line_2d"]).requires_grad_()
    p3 = _t(d["pts_3d"])             # no grad wanted
    l3 = _t(d["line_3d"]).requires_grad_()
    K = _t(d["K"]).requires_grad_()  # never differentiated
    R, t, status = pnpl_batch_diff(p2, l2, p3, l3, K)
    assert R.grad_fn is not None and not status.requires_grad
    rng = np.random.default_rng(0)
    gR, gt = _t(rng.standard_normal((512, 3, 3))), _t(rng.standard_normal((512, 3)))
    ((R * gR).sum() + (t * gt).sum()).backward()
    ref = pose_vjp(R.detach(), t.detach(), status, gR, gt, pts_2d=p2.detach(), line_2d=l2.detach(), pts_3d=p3, line_3d=l3.detach(), K=K.detach())
    torch.cuda.synchronize()
    assert torch.equal(p2.grad, ref["pts_2d"]) and torch.equal(l2.grad, ref["line_2d"]) and torch.equal(l3.grad, ref["line_3d"])
    assert p3.grad is None and K.grad is None
    assert (ref["vjp_status"] == (status != 0).int()).all()  # certified_only: the others are skipped


def test_diff_forward_is_bit_identical_to_pnpl_batch():
    for n_p, n_l, batch in ((10, 0, 3000), (0, 6, 500), (5, 5, 500), (2000, 0, 16)):
        d = synth.make_pnpl(batch, n_p, n_l, sigma=1.0, seed=n_p + n_l)
        a = [_t(d[k]) if (n_p if "pts" in k else n_l) else None for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")]
        ref = pnpl_batch(*a, _t(d["K"]))
        R, t, st = pnpl_batch_diff(*[x.requires_grad_() if x is not None else None for x in a], _t(d["K"]))
        assert torch.equal(R.detach(), ref.R) and torch.equal(t.detach(), ref.t) and torch.equal(st, ref.status)
    d = synth.make_pnp(300, 8, sigma=1.0, seed=3)
    R, t, st = pnp_batch_diff(_t(d["pts_2d"]), _t(d["pts_3d"]), _t(d["K"]))
    ref = pnpl_batch(_t(d["pts_2d"]), None, _t(d["pts_3d"]), None, _t(d["K"]))
    assert torch.equal(R, ref.R) and torch.equal(st, ref.status)
    d = synth.make_pnpl(300, 0, 8, sigma=1.0, seed=4)
    R, t, st = pnl_batch_diff(_t(d["line_2d"]), _t(d["line_3d"]), _t(d["K"]))
    ref = pnpl_batch(None, _t(d["line_2d"]), None, _t(d["line_3d"]), _t(d["K"]))
    assert torch.equal(t, ref.t) and torch.equal(st, ref.status)


def test_pixels_optimised_through_the_solver_recover_the_true_poses():
    """256 noisy PnP problems: 30 gradient-descent steps on the pixels (Polyak step size per problem: the loss is 0 at the true
    pixels) bring the mean pose error down at least ten-fold."""
    d = synth.make_pnp(256, 10, sigma=2.0, seed=7)
    x = _t(d["pts_2d"]).clone().requires_grad_()
    X, K, Rg, tg = _t(d["pts_3d"]), _t(d["K"]), _t(d["R_gt"]), _t(d["t_gt"])
    errs = []
    for it in range(31):
        R, t, status = pnp_batch_diff(x, X, K, certified_only=False)
        per = ((R - Rg) ** 2).sum((1, 2)) + ((t - tg) ** 2).sum(1)
        errs.append(per.detach().sqrt().mean().item())
        if it == 30:
            break
        x.grad = None
        per.sum().backward()
        with torch.no_grad():
            g = x.grad
            step = 0.5 * per.detach() / (g ** 2).sum((1, 2)).clamp_min(1e-300)
            x -= step[:, None, None] * g
    assert errs[-1] < 0.1 * errs[0], errs
