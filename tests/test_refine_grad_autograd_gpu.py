"""refine_pose_batch_diff: the forward is refine_pose_batch bit for bit, torch.autograd.grad of a linear loss is refine_vjp, a chained
pnp_batch_diff -> refine_pose_batch_diff graph is connected for every problem (a pose that passed through the refinement hands its upstream
gradient to the solve's backward unchanged), and inputs that do not require grad get None."""
import numpy as np
import pytest
import torch

from cvxpnpl_amd import synth

pytestmark = pytest.mark.gpu


def _problem(B=7, n=10, seed=5):
    d = synth.make_pnp(B, n, sigma=1.0, seed=seed)
    dev = torch.device("cuda")
    rs = np.random.RandomState(seed)
    as_dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)  # noqa: E731
    return (as_dev(d["pts_2d"]), as_dev(d["pts_3d"]), as_dev(d["K"]), as_dev(d["R_gt"]), as_dev(d["t_gt"] * 1.02), as_dev(rs.normal(size=(B, 3, 3))),
            as_dev(rs.normal(size=(B, 3))))


def test_forward_is_bit_identical_and_backward_is_refine_vjp():
    from cvxpnpl_amd import refine_pose_batch, refine_pose_batch_diff, refine_vjp

    p2, p3, K, R0, t0, GR, Gt = _problem()
    st = torch.tensor([0, 0, 1, 0, 2, 0, 0], dtype=torch.int32, device="cuda")         # problem 2 is not admitted: refine status 2
    plain = refine_pose_batch(R0, t0, pts_2d=p2, pts_3d=p3, K=K, status=st)
    a2, a3 = p2.clone().requires_grad_(True), p3.clone().requires_grad_(True)
    R0g, t0g = R0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    R, t, status = refine_pose_batch_diff(R0g, t0g, pts_2d=a2, pts_3d=a3, K=K, status=st)
    for x, y in ((R, plain.R), (t, plain.t), (status, plain.status)):
        assert x.detach().cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert status.cpu().tolist()[2] == 2 and not status.requires_grad and R.requires_grad and t.requires_grad
    loss = (GR * R).sum() + (Gt * t).sum()
    g2, g3, gR0, gt0 = torch.autograd.grad(loss, (a2, a3, R0g, t0g))
    want = refine_vjp(R.detach(), t.detach(), status, GR, Gt, pts_2d=p2, pts_3d=p3, K=K)
    assert (want["vjp_status"].cpu().numpy() == np.where(status.cpu().numpy() == 0, 0, 1)).all() and (status == 0).sum() >= 5
    assert g2.cpu().numpy().tobytes() == want["pts_2d"].cpu().numpy().tobytes() and g3.cpu().numpy().tobytes() == want["pts_3d"].cpu().numpy().tobytes()
    assert g2[0].abs().max() > 0 and not g2[2].any() and not g3[2].any()
    # the input pose: the upstream gradient where the pose passed through, zero where it was refined
    through = (status >= 2).cpu().numpy()
    assert through.tolist() == [False, False, True, False, False, False, False]
    assert torch.equal(gR0[2], GR[2]) and torch.equal(gt0[2], Gt[2])
    assert not gR0[~torch.as_tensor(through)].any() and not gt0[~torch.as_tensor(through)].any()
    # only t is used downstream, only pts_3d requires grad: the rest gets None
    b3 = p3.clone().requires_grad_(True)
    R, t, status = refine_pose_batch_diff(R0, t0, pts_2d=p2, pts_3d=b3, K=K, status=st)
    (g3t,) = torch.autograd.grad((Gt * t).sum(), (b3,))
    want = refine_vjp(R.detach(), t.detach(), status, None, Gt, pts_2d=p2, pts_3d=p3, K=K, want=("pts_3d",))
    assert g3t.cpu().numpy().tobytes() == want["pts_3d"].cpu().numpy().tobytes()
    Kg, c2 = K.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    R, t, status = refine_pose_batch_diff(R0, t0, pts_2d=c2, pts_3d=p3, K=Kg, status=st)
    gK, gc2 = torch.autograd.grad((GR * R).sum(), (Kg, c2), allow_unused=True)
    assert gK is None and gc2 is not None
    R, t, status = refine_pose_batch_diff(R0, t0, pts_2d=p2, pts_3d=p3, K=K)
    assert not R.requires_grad and not t.requires_grad


def test_chained_with_the_solve_the_graph_is_connected_for_every_problem():
    from cvxpnpl_amd import pnp_batch_diff, pose_passthrough, pose_vjp, refine_pose_batch_diff, refine_vjp

    p2, p3, K, _, _, GR, Gt = _problem(B=9, seed=8)
    a2 = p2.clone().requires_grad_(True)
    R0, t0, st0 = pnp_batch_diff(a2, p3, K)
    cert = (st0 == 0).cpu().numpy()
    assert cert.sum() >= 7, st0
    forced = int(np.flatnonzero(cert)[1])                         # a certified problem whose refinement is switched off through `status`
    st_in = st0.clone()
    st_in[forced] = 1                                             # rank > 1: not in the refinement's admit mask
    R, t, status = refine_pose_batch_diff(R0, t0, pts_2d=a2, pts_3d=p3, K=K, status=st_in)
    rs = status.cpu().numpy()
    assert rs[forced] == 2 and (rs[np.flatnonzero(cert)[np.flatnonzero(cert) != forced]] == 0).all(), rs
    assert torch.equal(R[forced], R0[forced]) and torch.equal(t[forced], t0[forced])
    (g,) = torch.autograd.grad((GR * R).sum() + (Gt * t).sum(), (a2,))
    from_refine = refine_vjp(R.detach(), t.detach(), status, GR, Gt, pts_2d=p2, pts_3d=p3, K=K, want=("pts_2d",))["pts_2d"]
    pR, pt = pose_passthrough(status, GR, Gt)
    from_solve = pose_vjp(R0.detach(), t0.detach(), st0, pR, pt, pts_2d=p2, pts_3d=p3, K=K, want=("pts_2d",))["pts_2d"]
    assert from_solve[forced].abs().max() > 0 and not from_refine[forced].any()
    assert torch.equal(g[forced], from_solve[forced])             # exactly what pose_vjp gives for the problem that passed through
    others = [b for b in range(9) if b != forced]
    assert torch.equal(g[others], from_refine[others])            # exactly what refine_vjp gives for the others
    assert g[np.flatnonzero(cert)].abs().amax(dim=(1, 2)).min() > 0      # every certified problem receives a gradient
