"""refine_pose_batch_robust_diff: the forward is refine_pose_batch_robust bit for bit, torch.autograd.grad of a linear loss is
refine_vjp_robust for all six inputs, a chained pnp_batch_diff -> refine_pose_batch_robust_diff graph is connected for every problem,
and requires_grad on the weights alone returns the weights' gradients alone."""
import numpy as np
import pytest
import torch

from cvxpnpl_amd import synth

pytestmark = pytest.mark.gpu

# Under Huber and Cauchy the forward converges linearly and may use up its default 30 trials: the tests give it 100
# and differentiate converged and max_iters poses alike
FWD = dict(max_iters=100)
ADMIT = 0x3


def as_dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _problem(B=7, n_p=8, n_l=5, seed=5):
    d = synth.make_pnpl(B, n_p, n_l, 1.0, seed=seed)
    rs = np.random.RandomState(seed)
    return dict(p2=as_dev(d["pts_2d"]), p3=as_dev(d["pts_3d"]), l2=as_dev(d["line_2d"]), l3=as_dev(d["line_3d"]), K=as_dev(d["K"]), R0=as_dev(d["R_gt"]),
                t0=as_dev(d["t_gt"] * 1.02), GR=as_dev(rs.normal(size=(B, 3, 3))), Gt=as_dev(rs.normal(size=(B, 3))),
                wp=as_dev(rs.uniform(0.25, 4.0, (B, n_p))), wl=as_dev(rs.uniform(0.25, 4.0, (B, n_l))))


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_forward_is_bit_identical_and_backward_is_refine_vjp_robust(loss):
    from cvxpnpl_amd import refine_pose_batch_robust, refine_pose_batch_robust_diff, refine_vjp_robust

    p = _problem()
    st = torch.tensor([0, 0, 1, 0, 2, 0, 0], dtype=torch.int32, device="cuda")         # problem 2 is not admitted: refine status 2
    data = dict(pts_2d=p["p2"], line_2d=p["l2"], pts_3d=p["p3"], line_3d=p["l3"], weights_pts=p["wp"], weights_lines=p["wl"])
    plain = refine_pose_batch_robust(p["R0"], p["t0"], K=p["K"], loss=loss, scale_px=1.0, status=st, **FWD, **data)
    leaves = {k: v.clone().requires_grad_(True) for k, v in data.items()}
    R0g, t0g = p["R0"].clone().requires_grad_(True), p["t0"].clone().requires_grad_(True)
    R, t, status = refine_pose_batch_robust_diff(R0g, t0g, K=p["K"], loss=loss, scale_px=1.0, status=st, admit_mask=ADMIT, **FWD, **leaves)
    for x, y in ((R, plain.R), (t, plain.t), (status, plain.status)):
        assert x.detach().cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert status.cpu().tolist()[2] == 2 and not status.requires_grad and R.requires_grad and t.requires_grad
    L = (p["GR"] * R).sum() + (p["Gt"] * t).sum()
    names = list(leaves)
    grads = torch.autograd.grad(L, [leaves[k] for k in names] + [R0g, t0g])
    want = refine_vjp_robust(R.detach(), t.detach(), status, p["GR"], p["Gt"], K=p["K"], loss=loss, scale_px=1.0, admit_mask=ADMIT, **data)
    assert (want["vjp_status"].cpu().numpy() == np.where(status.cpu().numpy() <= 1, 0, 1)).all() and (status <= 1).sum() >= 5
    for k, g in zip(names, grads):
        assert g.shape == data[k].shape and g.cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
        assert g[0].abs().max() > 0 and not g[2].any(), k
    gR0, gt0 = grads[-2:]
    assert torch.equal(gR0[2], p["GR"][2]) and torch.equal(gt0[2], p["Gt"][2])          # the pose that passed through
    keep = torch.arange(7, device="cuda") != 2
    assert not gR0[keep].any() and not gt0[keep].any()
    # K, loss, scale, masks, status: None; an input that does not require grad: no gradient asked of the kernels
    Kg = p["K"].clone().requires_grad_(True)
    R, t, status = refine_pose_batch_robust_diff(p["R0"], p["t0"], K=Kg, loss=loss, scale_px=1.0, status=st, **FWD, **dict(data, pts_2d=leaves["pts_2d"]))
    gK, g2 = torch.autograd.grad((p["GR"] * R).sum(), (Kg, leaves["pts_2d"]), allow_unused=True)
    assert gK is None and g2 is not None
    R, t, status = refine_pose_batch_robust_diff(p["R0"], p["t0"], K=p["K"], loss=loss, scale_px=1.0, **data)
    assert not R.requires_grad and not t.requires_grad


def test_requires_grad_on_the_weights_alone_returns_the_weights_gradients_alone(monkeypatch):
    from cvxpnpl_amd import refine_robust_grad as rg

    p = _problem(seed=9)
    wp, wl = p["wp"].clone().requires_grad_(True), p["wl"].clone().requires_grad_(True)
    seen = []
    real = rg.refine_vjp_robust

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw["want"], [k for k in rg.ROBUST_GRAD_NAMES if out[k] is not None]))
        return out

    monkeypatch.setattr(rg, "refine_vjp_robust", spy)
    R, t, status = rg.refine_pose_batch_robust_diff(p["R0"], p["t0"], pts_2d=p["p2"], line_2d=p["l2"], pts_3d=p["p3"], line_3d=p["l3"], K=p["K"], loss="cauchy",
                                                    scale_px=1.0, weights_pts=wp, weights_lines=wl, admit_mask=ADMIT, **FWD)
    gwp, gwl = torch.autograd.grad((p["Gt"] * t).sum(), (wp, wl))
    assert seen == [(("weights_pts", "weights_lines"), ["weights_pts", "weights_lines"])], seen
    want = real(R.detach(), t.detach(), status, None, p["Gt"], pts_2d=p["p2"], line_2d=p["l2"], pts_3d=p["p3"], line_3d=p["l3"], K=p["K"], loss="cauchy",
                scale_px=1.0, weights_pts=p["wp"], weights_lines=p["wl"], admit_mask=ADMIT, want=("weights_pts", "weights_lines"))
    assert gwp.cpu().numpy().tobytes() == want["weights_pts"].cpu().numpy().tobytes() and gwl.cpu().numpy().tobytes() == want["weights_lines"].cpu().numpy().tobytes()
    assert gwp.abs().min() > 0 and (status <= 1).all()
    # a confidence that reaches exactly 0 stays there
    w0 = p["wp"].clone()
    w0[:, 3] = 0.0
    w0.requires_grad_(True)
    R, t, status = rg.refine_pose_batch_robust_diff(p["R0"], p["t0"], pts_2d=p["p2"], line_2d=p["l2"], pts_3d=p["p3"], line_3d=p["l3"], K=p["K"], loss="huber",
                                                    scale_px=1.0, weights_pts=w0, weights_lines=p["wl"], admit_mask=ADMIT, **FWD)
    (g0,) = torch.autograd.grad((p["GR"] * R).sum(), (w0,))
    assert not g0[:, 3].any() and g0[:, :3].abs().min() > 0


def test_chained_with_the_solve_the_graph_is_connected_for_every_problem():
    from cvxpnpl_amd import pnp_batch_diff, pose_passthrough, pose_vjp, refine_pose_batch_robust_diff, refine_vjp_robust

    d = synth.make_pnp(9, 10, sigma=1.0, seed=8)
    rs = np.random.RandomState(8)
    p2, p3, K = as_dev(d["pts_2d"]), as_dev(d["pts_3d"]), as_dev(d["K"])
    GR, Gt, w = as_dev(rs.normal(size=(9, 3, 3))), as_dev(rs.normal(size=(9, 3))), as_dev(rs.uniform(0.25, 4.0, (9, 10)))
    a2 = p2.clone().requires_grad_(True)
    R0, t0, st0 = pnp_batch_diff(a2, p3, K)
    cert = (st0 == 0).cpu().numpy()
    assert cert.sum() >= 7, st0
    forced = int(np.flatnonzero(cert)[1])                         # a certified problem whose refinement is switched off through `status`
    st_in = st0.clone()
    st_in[forced] = 1                                             # rank > 1: not in the refinement's admit mask
    R, t, status = refine_pose_batch_robust_diff(R0, t0, pts_2d=a2, pts_3d=p3, K=K, loss="huber", scale_px=1.0, weights_pts=w, status=st_in, admit_mask=ADMIT,
                                                 **FWD)
    rs_ = status.cpu().numpy()
    assert rs_[forced] == 2 and (rs_[np.flatnonzero(cert)[np.flatnonzero(cert) != forced]] <= 1).all(), rs_
    assert torch.equal(R[forced], R0[forced]) and torch.equal(t[forced], t0[forced])
    (g,) = torch.autograd.grad((GR * R).sum() + (Gt * t).sum(), (a2,))
    from_refine = refine_vjp_robust(R.detach(), t.detach(), status, GR, Gt, pts_2d=p2, pts_3d=p3, K=K, loss="huber", scale_px=1.0, weights_pts=w,
                                    admit_mask=ADMIT, want=("pts_2d",))["pts_2d"]
    pR, pt = pose_passthrough(status, GR, Gt)
    from_solve = pose_vjp(R0.detach(), t0.detach(), st0, pR, pt, pts_2d=p2, pts_3d=p3, K=K, want=("pts_2d",))["pts_2d"]
    assert from_solve[forced].abs().max() > 0 and not from_refine[forced].any()
    assert torch.equal(g[forced], from_solve[forced])             # exactly what pose_vjp gives for the problem that passed through
    others = [b for b in range(9) if b != forced]
    assert torch.equal(g[others], from_refine[others])            # exactly what refine_vjp_robust gives for the others
    assert g[np.flatnonzero(cert)].abs().amax(dim=(1, 2)).min() > 0
