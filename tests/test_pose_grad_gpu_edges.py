"""The device-only logic of the pose VJP (vjp_kernel.h, grad_hip.hip) at its edges, and the kernels against an independent
reference (-m gpu).  Inputs are seeded synth data; statuses are ASSIGNED by the test, so that every status occurs in both regimes
(16 lanes per problem below 768 records; reduce -> solve -> scatter from 768 on).  No forward solve except in the autograd tests.

Two kinds of assertion:

* device vs reference (grad_reference.reference_vjp: float64 autograd of the cost's definition, nothing of the product), at poses
  polished on the CPU, relative L2 per problem over all four gradients.  Measured on the MI355X over the cases of
  test_device_matches_the_autograd_reference: worst error 1.16e-14 (pnp10; 1.1e-14 for pnp4, below 5e-15 for every other case, below
  2e-15 in the multi-block path).  The host twin's worst over the same problems is 1.4e-14: the kernels add nothing to it.
  DEV_BOUND = 1.2e-12 = 100 x the worst, because the error grows with cond(H).
* device vs host twin to the project's 1e-10 (TWIN), with exact agreement of vjp_status, zeros for every problem that is not
  VJP_OK and NaN info for skipped ones: the regime boundary, the tails of the 16-problem workgroups and the 64-lane solve kernel,
  1 ... 33 correspondences per 16-lane group, absent arguments and outputs, more than ten partial blocks, and 65 536 problems of 768
  points through the group-kernel fallback.

Plus what only a device can get wrong: a side stream with back-to-back calls of different sizes (stream-ordered scratch), and the
same call twice giving the same bits.
"""
import numpy as np
import pytest
import torch

import grad_reference as gr
from cvxpnpl_amd import synth
from cvxpnpl_amd.grad import ADMIT_CERTIFIED, ADMIT_RANK1, pnp_batch_diff, pnpl_batch_diff, pose_vjp, pose_vjp_host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = gr.NAMES
TWIN = 1e-10       # device vs host twin (the bound of test_pose_grad_gpu.py)
DEV_BOUND = 1.2e-12  # device vs reference: 100 x the worst error measured on the MI355X (1.16e-14)
CYCLE = np.array([0, 1, 2, 3, 4], np.int32)


def _t(x):
    return torch.as_tensor(x, device=DEV) if x is not None else None


def _sync():
    torch.cuda.synchronize()


def _scene(batch, n_p, n_l, seed, sigma=1.0):
    d = synth.make_pnpl(batch, n_p, n_l, sigma=sigma, seed=seed)
    rng = np.random.default_rng(seed)
    d["gR"], d["gt"] = rng.standard_normal((batch, 3, 3)), rng.standard_normal((batch, 3))
    return d


def _device(d, R, t, status, gR, gt, **kw):
    """pose_vjp on the arrays of d; everything back on the host as numpy."""
    out = pose_vjp(_t(R), _t(t), _t(status), _t(gR), _t(gt), K=_t(d["K"]), **{k: _t(v) for k, v in gr.kinds(d).items()}, **kw)
    _sync()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _assert_twin(dev, host, want=NAMES, expect_status=None, tag=""):
    """Device result against the host twin's: statuses exact, the wanted gradients to TWIN for VJP_OK problems and exactly zero for the
    others, unwanted ones absent.  Returns the worst relative error."""
    vst = dev["vjp_status"]
    assert np.array_equal(vst, host["vjp_status"]), (tag, vst, host["vjp_status"])
    if expect_status is not None:
        assert np.array_equal(vst, np.asarray(expect_status)), (tag, vst, expect_status)
    batch = len(vst)
    num, den = np.zeros(batch), np.zeros(batch)
    for name in NAMES:
        if host[name] is None or name not in want:
            assert dev.get(name) is None, (tag, name)
            continue
        a, b = dev[name].reshape(batch, -1), host[name].reshape(batch, -1)
        assert a.shape == b.shape and np.isfinite(a).all(), (tag, name)
        assert not a[vst != 0].any() and not b[vst != 0].any(), (tag, name)
        num += ((a - b) ** 2).sum(1)
        den += (b ** 2).sum(1)
    ok = vst == 0
    if "info" in dev:
        assert np.isnan(dev["info"][vst == 1]).all(), tag
        assert np.allclose(dev["info"][ok, 0], host["info"][ok, 0], rtol=1e-6), tag
        assert np.allclose(dev["info"][ok, 1], host["info"][ok, 1], rtol=1e-3, atol=1e-11), tag
    if not ok.any():
        return 0.0
    assert (den[ok] > 0).all(), tag
    rel = np.sqrt(num[ok] / den[ok])
    assert rel.max() < TWIN, (tag, rel.max(), int(np.argmax(rel)))
    return float(rel.max())


def _expected(status, admit):
    return np.where((admit >> status) & 1, 0, 1).astype(np.int32)


def _twin_case(batch, n_p, n_l, seed, admit=ADMIT_RANK1, info=True, expect_ok=True):
    """Ground-truth poses of noisy data (device == host needs no stationary pose), statuses 0 1 2 3 4 0 ... assigned."""
    d = _scene(batch, n_p, n_l, seed)
    status = CYCLE[np.arange(batch) % 5]
    dev = _device(d, d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], admit_mask=admit, want_info=info)
    host = pose_vjp_host(d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], K=d["K"], admit_mask=admit, **gr.kinds(d))
    tag = f"batch {batch}, {n_p} points + {n_l} lines"
    return _assert_twin(dev, host, expect_status=_expected(status, admit) if expect_ok else None, tag=tag)


# ---------------------------------------------------------------------------------------------- device vs the reference
def _reference_errors(d, R, t, status, admit, idx):
    dev = _device(d, R, t, status, d["gR"], d["gt"], admit_mask=admit)
    assert (dev["vjp_status"] == 0).all(), dev["vjp_status"]
    errs = []
    for b in idx:
        p2, p3, l2, l3, K = gr.problem(d, b)
        truth = gr.flat(gr.reference_vjp(R[b], t[b], p2, p3, l2, l3, K, d["gR"][b], d["gt"][b], gr.records(p3, l3).mean(0)))
        errs.append(gr.rel_err(gr.flat(dev, b), truth))
    return np.array(errs)


REFERENCE_CASES = {  # name: (batch, n_p, n_l, seed, per-problem K, reflected)
    "pnp4": (32, 4, 0, 201, False, False), "pnp10": (32, 10, 0, 202, False, False), "pnp17": (32, 17, 0, 203, False, False),
    "pnpl5+5": (32, 5, 5, 204, False, False), "pnp10-Kper": (32, 10, 0, 205, True, False), "pnpl5+5-Kper": (16, 5, 5, 206, True, False),
    "pnp10-reflected": (32, 10, 0, 207, False, True), "pnpl5+5-reflected": (16, 5, 5, 208, False, True),
    "pnp900": (6, 900, 0, 209, False, False), "pnpl300+300": (4, 300, 300, 210, False, False), "pnp2000-2blocks": (3, 2000, 0, 211, False, False),
    "pnp900-reflected": (3, 900, 0, 212, False, True),
}


@pytest.mark.parametrize("name", list(REFERENCE_CASES))
def test_device_matches_the_autograd_reference(name):
    batch, n_p, n_l, seed, K_per, reflected = REFERENCE_CASES[name]
    d = _scene(batch, n_p, n_l, seed, sigma=2.0)
    if K_per:
        d = gr.per_problem_K(d, seed)
    R, t, g, fit = gr.polish_batch(d)
    good = (g < 1e-12) | (fit < 1e-13)
    assert (~good).sum() <= 0.05 * batch, (g, fit)
    if reflected:  # det R = -1: a stationary point all the same (f is even in (R, t)); what ADMIT_RANK1 admits as CVXPNPL_REFLECTION
        R, t = -R, -t
    status = np.full(batch, 4 if reflected else 0, np.int32)
    errs = _reference_errors(d, R, t, status, ADMIT_RANK1 if reflected else ADMIT_CERTIFIED, np.flatnonzero(good))
    print(f"{name}: {good.sum()} problems, worst device-vs-reference {errs.max():.2e}")
    assert errs.max() < DEV_BOUND, (name, errs)


# ---------------------------------------------------------------------------------------------- device vs host: shapes and tails
BOUNDARY = [(767, 0), (768, 0), (0, 383), (0, 384), (101, 333), (100, 334), (1, 383), (766, 1)]


@pytest.mark.parametrize("n_p,n_l", BOUNDARY, ids=[f"{p}+{l}" for p, l in BOUNDARY])
def test_regime_boundary_by_points_lines_and_a_mix(n_p, n_l):
    """records = n_p + 2 n_l at 767 | 768: the last shape of the group kernel and the first of the multi-block path."""
    for batch in (1, 7):
        _twin_case(batch, n_p, n_l, seed=300 + n_p + n_l)


@pytest.mark.parametrize("batch", [1, 2, 15, 16, 17, 31, 33, 63, 64, 65])
def test_batch_tails_small_n(batch):
    """16 problems per workgroup, four per wavefront: the partly filled last workgroup and wavefront."""
    for n_p, n_l in ((10, 0), (3, 4)):
        _twin_case(batch, n_p, n_l, seed=400 + batch)


@pytest.mark.parametrize("batch", [1, 2, 15, 17, 63, 64, 65, 129])
def test_batch_tails_large_n(batch):
    """One lane per problem in the 64-lane solve kernel; blockIdx.y = problem in the reduction; the scatter's flat index."""
    _twin_case(batch, 800, 0, seed=500 + batch)
    if batch in (1, 65):
        _twin_case(batch, 100, 350, seed=600 + batch)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 15, 16, 17, 31, 32, 33])
def test_correspondence_counts_around_the_group_width(n):
    """Lane l of a 16-lane group takes correspondences l, l + 16, ...: idle lanes, one trip, two trips, a third for one lane.  Fewer
    than three correspondences are VJP_SINGULAR (vjp_core.h: solve_v) on both sides."""
    few = n < 3
    for n_p, n_l in ((n, 0), (0, n), (n // 2, n - n // 2)):
        d = _scene(37, n_p, n_l, seed=700 + n)
        status = CYCLE[np.arange(37) % 5]
        dev = _device(d, d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], admit_mask=ADMIT_RANK1, want_info=True)
        host = pose_vjp_host(d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], K=d["K"], admit_mask=ADMIT_RANK1, **gr.kinds(d))
        expect = _expected(status, ADMIT_RANK1)
        if few:
            expect = np.where(expect == 0, 2, expect)
        if n == 3:  # a minimal problem at a pose that is not stationary: H may be indefinite, so only device == host is asserted
            expect = None
        _assert_twin(dev, host, expect_status=expect, tag=f"{n_p}+{n_l}")


def test_more_than_ten_partial_blocks():
    """batch 1 x 50 000 points: vjp_blocks = 49 (the other large-N tests run 1, 2 and 10); and 3 x 20 000: 20."""
    _twin_case(1, 50_000, 0, seed=801)
    _twin_case(3, 20_000, 0, seed=802)
    _twin_case(2, 6000, 3000, seed=803)


# ---------------------------------------------------------------------------------------------- statuses in the large-N path
def _mixed_batch(n_p, n_l, seed):
    """12 problems, statuses 0 1 2 3 4 0 ...; problem 5 (status 0) has a NaN pose, problem 10 (status 0) a collinear noise-free scene."""
    d = _scene(12, n_p, n_l, seed)
    status = CYCLE[np.arange(12) % 5]
    R, t = d["R_gt"].copy(), d["t_gt"].copy()
    R[5, 1, 2] = np.nan
    s = np.linspace(-0.3, 0.3, n_p + 2 * n_l)
    P = np.stack([s, 0.5 * s + 0.01, -0.2 * s], 1)[None]
    x = synth.project(P, d["K"], R[10:11], t[10:11])
    d["pts_3d"][10], d["pts_2d"][10] = P[0, :n_p], x[0, :n_p]
    d["line_3d"][10], d["line_2d"][10] = P[0, n_p:].reshape(n_l, 2, 3), x[0, n_p:].reshape(n_l, 2, 2)
    return d, R, t, status


@pytest.mark.parametrize("n_p,n_l", [(900, 0), (300, 300), (10, 0), (5, 5)], ids=["large-900", "large-300+300", "small-10", "small-5+5"])
@pytest.mark.parametrize("admit", [ADMIT_CERTIFIED, ADMIT_RANK1], ids=["certified", "rank1"])
def test_skipped_singular_and_nonfinite_problems_in_one_batch(n_p, n_l, admit):
    """Every status in one batch of the multi-block path (and of the group kernel): skipped, singular and non-finite problems get
    all-zero gradients, skipped ones NaN info, and their neighbours are untouched -- bit for bit what they are in a batch where every
    problem is differentiated (the early return of the reduction leaves rows of the partial sums unwritten; nobody may read them)."""
    d, R, t, status = _mixed_batch(n_p, n_l, seed=900 + n_p)
    expect = _expected(status, admit)
    if expect[5] == 0:
        expect[5] = 3
    if expect[10] == 0:
        expect[10] = 2
    dev = _device(d, R, t, status, d["gR"], d["gt"], admit_mask=admit, want_info=True)
    host = pose_vjp_host(R, t, status, d["gR"], d["gt"], K=d["K"], admit_mask=admit, **gr.kinds(d))
    _assert_twin(dev, host, expect_status=expect, tag="mixed")
    assert (expect == 0).any() and {1, 2, 3} <= set(expect.tolist())
    clean = _device(d, d["R_gt"], d["t_gt"], None, d["gR"], d["gt"], want_info=True)
    for b in np.flatnonzero(expect == 0):
        for name in NAMES:
            if dev[name] is not None:
                assert np.array_equal(dev[name][b], clean[name][b]), (b, name)
        assert np.array_equal(dev["info"][b], clean["info"][b]), b


# ---------------------------------------------------------------------------------------------- absent arguments and outputs
@pytest.mark.parametrize("batch,n_p,n_l", [(33, 6, 5), (5, 500, 200)], ids=["small", "large"])
def test_absent_status_and_upstream_gradients(batch, n_p, n_l):
    d = _scene(batch, n_p, n_l, seed=1000 + batch)
    R, t, gR, gt = d["R_gt"], d["t_gt"], d["gR"], d["gt"]
    status = CYCLE[np.arange(batch) % 5]
    hk = dict(K=d["K"], **gr.kinds(d))
    for tag, st, a, b in (("status=None", None, gR, gt), ("grad_R=None", status, None, gt), ("grad_t=None", status, gR, None),
                          ("both None", status, None, None)):
        for admit in (ADMIT_CERTIFIED, ADMIT_RANK1):
            dev = _device(d, R, t, st, a, b, admit_mask=admit, want_info=True)
            host = pose_vjp_host(R, t, st, a, b, admit_mask=admit, **hk)
            expect = np.zeros(batch, np.int32) if st is None else _expected(status, admit)
            if tag == "both None":  # b = 0: v = 0 and every gradient is exactly zero, on both sides
                assert np.array_equal(dev["vjp_status"], expect) and np.array_equal(host["vjp_status"], expect)
                assert not gr.flat(dev).any() and not gr.flat(host).any()
            else:
                _assert_twin(dev, host, expect_status=expect, tag=tag)
    # None is zero, bit for bit
    zR = _device(d, R, t, status, np.zeros_like(gR), gt, admit_mask=ADMIT_RANK1)
    nR = _device(d, R, t, status, None, gt, admit_mask=ADMIT_RANK1)
    zt = _device(d, R, t, status, gR, np.zeros_like(gt), admit_mask=ADMIT_RANK1)
    nt = _device(d, R, t, status, gR, None, admit_mask=ADMIT_RANK1)
    assert np.array_equal(gr.flat(zR), gr.flat(nR)) and np.array_equal(gr.flat(zt), gr.flat(nt))


@pytest.mark.parametrize("batch,n_p,n_l", [(33, 6, 5), (5, 500, 200)], ids=["small", "large"])
def test_each_single_wanted_output(batch, n_p, n_l):
    d = _scene(batch, n_p, n_l, seed=1100 + batch)
    status = CYCLE[np.arange(batch) % 5]
    full = _device(d, d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], admit_mask=ADMIT_RANK1)
    host = pose_vjp_host(d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], K=d["K"], admit_mask=ADMIT_RANK1, **gr.kinds(d))
    _assert_twin(full, host, expect_status=_expected(status, ADMIT_RANK1))
    for want in [(n,) for n in NAMES] + [("pts_2d", "line_3d"), ()]:
        one = _device(d, d["R_gt"], d["t_gt"], status, d["gR"], d["gt"], admit_mask=ADMIT_RANK1, want=want)
        assert np.array_equal(one["vjp_status"], full["vjp_status"]), want
        for name in NAMES:
            if name in want:
                assert np.array_equal(one[name], full[name]), (want, name)  # the other outputs' absence changes no bit
            else:
                assert one[name] is None, (want, name)


def test_points_only_and_lines_only_leave_the_other_kind_none():
    for n_p, n_l in ((10, 0), (0, 10), (800, 0), (0, 400)):
        d = _scene(5, n_p, n_l, seed=1200 + n_p)
        dev = _device(d, d["R_gt"], d["t_gt"], None, d["gR"], d["gt"])
        host = pose_vjp_host(d["R_gt"], d["t_gt"], None, d["gR"], d["gt"], K=d["K"], **gr.kinds(d))
        _assert_twin(dev, host, expect_status=np.zeros(5, np.int32))
        assert (dev["pts_2d"] is None) == (n_p == 0) and (dev["line_3d"] is None) == (n_l == 0)


# ---------------------------------------------------------------------------------------------- the group-kernel fallback
def test_65536_problems_of_768_points_fall_back_to_the_group_kernel():
    """More problems than one grid dimension holds, with 768 records each: vjp_group_kernel, every lane looping 48 times.  The data is
    generated on the device (about 2 GB of correspondences and 0.8 GB of gradients); the host twin checks a 256-problem sample plus
    the first and the last problem."""
    batch, n = 65_536, 768
    d = synth.device_pnpl(batch, n, 0, sigma=1.0, seed=65536, device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(1)
    gR = torch.randn((batch, 3, 3), generator=gen, dtype=torch.float64).to(DEV)
    gt = torch.randn((batch, 3), generator=gen, dtype=torch.float64).to(DEV)
    status = torch.arange(batch, device=DEV, dtype=torch.int32) % 5
    out = pose_vjp(d["R_gt"], d["t_gt"], status, gR, gt, pts_2d=d["pts_2d"], pts_3d=d["pts_3d"], K=d["K"], admit_mask=ADMIT_RANK1,
                   want=("pts_2d",))
    _sync()
    assert out["pts_3d"] is None and out["pts_2d"].shape == (batch, n, 2)
    vst = out["vjp_status"].cpu().numpy()
    assert np.array_equal(vst, _expected((np.arange(batch) % 5).astype(np.int32), ADMIT_RANK1))
    idx = np.unique(np.concatenate([[0, batch - 1], np.random.default_rng(2).choice(batch, 256, replace=False)]))
    ti = torch.as_tensor(idx, device=DEV)
    pick = lambda x: x[ti].cpu().numpy()  # noqa: E731
    host = pose_vjp_host(pick(d["R_gt"]), pick(d["t_gt"]), pick(status), pick(gR), pick(gt), pts_2d=pick(d["pts_2d"]), pts_3d=pick(d["pts_3d"]),
                         K=d["K"].cpu().numpy(), admit_mask=ADMIT_RANK1, n_threads=16)
    dev = {"pts_2d": pick(out["pts_2d"]), "pts_3d": None, "line_2d": None, "line_3d": None, "vjp_status": vst[idx]}
    _assert_twin(dev, host, want=("pts_2d",), tag="65536 x 768")
    # skipped problems are zero everywhere, not only in the sample
    skipped = torch.as_tensor(vst != 0, device=DEV)
    assert not out["pts_2d"][skipped].any() and torch.isfinite(out["pts_2d"]).all()


# ---------------------------------------------------------------------------------------------- streams and determinism
def _call(d, status, want_info=False):
    return pose_vjp(d["R"], d["t"], status, d["gR_d"], d["gt_d"], K=d["K_d"], admit_mask=ADMIT_RANK1, want_info=want_info, **d["dev"])


def _resident(batch, n_p, n_l, seed):
    d = _scene(batch, n_p, n_l, seed)
    d["R"], d["t"], d["gR_d"], d["gt_d"], d["K_d"] = _t(d["R_gt"]), _t(d["t_gt"]), _t(d["gR"]), _t(d["gt"]), _t(d["K"])
    d["dev"] = {k: _t(v) for k, v in gr.kinds(d).items()}
    d["status"] = _t(CYCLE[np.arange(batch) % 5])
    return d


def _same(a, b):
    for k in list(NAMES) + ["vjp_status"]:
        if a[k] is None:
            assert b[k] is None
        else:
            assert torch.equal(a[k], b[k]), k


def test_side_stream_back_to_back_calls_of_different_sizes():
    """The large-N path allocates and frees its scratch in stream order: a large call, a small one and a larger one queued on a side
    stream with no host synchronisation in between give the bits of the default stream."""
    jobs = [_resident(9, 1500, 0, 1301), _resident(200, 10, 3, 1302), _resident(3, 20_000, 0, 1303), _resident(40, 300, 300, 1304)]
    _sync()
    ref = [_call(d, d["status"]) for d in jobs]
    _sync()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = [_call(d, d["status"]) for d in jobs]
        again = [_call(d, d["status"]) for d in reversed(jobs)][::-1]
    side.synchronize()
    for a, b, c in zip(ref, got, again):
        _same(a, b)
        _same(a, c)
    _sync()


@pytest.mark.parametrize("batch,n_p,n_l", [(7, 3000, 0), (64, 400, 200), (1, 50_000, 0), (1000, 10, 0), (500, 5, 5), (3, 600, 80)],
                         ids=["large-7x3000", "large-64x400+200", "large-49-blocks", "group-10", "group-5+5", "group-600+80"])
def test_the_same_call_twice_gives_the_same_bits(batch, n_p, n_l):
    d = _resident(batch, n_p, n_l, 1400 + batch)
    a = _call(d, d["status"], want_info=True)
    b = _call(d, d["status"], want_info=True)
    _sync()
    _same(a, b)
    assert torch.equal(a["info"].nan_to_num(nan=-1.0), b["info"].nan_to_num(nan=-1.0))


# ---------------------------------------------------------------------------------------------- the autograd wrapper
def _loss(R, t, gR, gt):
    return (R * gR).sum() + (t * gt).sum()


def test_float32_leaves_get_float32_gradients_of_the_upcast_inputs():
    d = _scene(256, 6, 4, seed=1501)
    leaves = [_t(d[k]).float().requires_grad_() for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")]
    R, t, status = pnpl_batch_diff(*leaves, _t(d["K"]).float())
    assert R.dtype == torch.float64 and (status == 0).float().mean() > 0.5
    gR, gt = _t(d["gR"]), _t(d["gt"])
    _loss(R, t, gR, gt).backward()
    up = [x.detach().double() for x in leaves]
    ref = pose_vjp(R.detach(), t.detach(), status, gR, gt, pts_2d=up[0], line_2d=up[1], pts_3d=up[2], line_3d=up[3], K=_t(d["K"]).float().double())
    _sync()
    for x, name in zip(leaves, ("pts_2d", "line_2d", "pts_3d", "line_3d")):
        assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
        assert torch.equal(x.grad, ref[name].float()), name
        assert x.grad[status == 0].abs().max() > 0


def test_non_contiguous_leaf_gets_a_gradient_of_its_own_shape():
    d = _scene(256, 8, 0, seed=1502)
    wide2 = torch.zeros((256, 8, 5), device=DEV, dtype=torch.float64)
    wide2[..., 1:3] = _t(d["pts_2d"])
    wide3 = torch.zeros((256, 3, 8), device=DEV, dtype=torch.float64)
    wide3[:] = _t(d["pts_3d"]).transpose(1, 2)
    p2 = wide2[..., 1:3].detach().requires_grad_()         # a slice of a wider tensor
    p3 = wide3.transpose(1, 2).detach().requires_grad_()   # a transposed view
    assert not p2.is_contiguous() and not p3.is_contiguous()
    c2, c3 = _t(d["pts_2d"]).requires_grad_(), _t(d["pts_3d"]).requires_grad_()
    gR, gt = _t(d["gR"]), _t(d["gt"])
    R, t, st = pnp_batch_diff(p2, p3, _t(d["K"]))
    _loss(R, t, gR, gt).backward()
    Rc, tc, stc = pnp_batch_diff(c2, c3, _t(d["K"]))
    _loss(Rc, tc, gR, gt).backward()
    assert torch.equal(R, Rc) and torch.equal(st, stc)
    assert p2.grad.shape == p2.shape and p3.grad.shape == p3.shape
    assert torch.equal(p2.grad, c2.grad) and torch.equal(p3.grad, c3.grad) and c2.grad.abs().max() > 0


def test_numpy_inputs_beside_tensor_leaves():
    d = _scene(128, 5, 5, seed=1503)
    p2, l2 = _t(d["pts_2d"]).requires_grad_(), _t(d["line_2d"]).requires_grad_()
    R, t, st = pnpl_batch_diff(p2, l2, d["pts_3d"], d["line_3d"], d["K"])  # numpy: never differentiated, needed in the backward all the same
    gR, gt = _t(d["gR"]), _t(d["gt"])
    _loss(R, t, gR, gt).backward()
    ref = pose_vjp(R.detach(), t.detach(), st, gR, gt, pts_2d=p2.detach(), line_2d=l2.detach(), pts_3d=_t(d["pts_3d"]), line_3d=_t(d["line_3d"]),
                   K=_t(d["K"]), want=("pts_2d", "line_2d"))
    _sync()
    assert torch.equal(p2.grad, ref["pts_2d"]) and torch.equal(l2.grad, ref["line_2d"]) and p2.grad.abs().max() > 0


def test_loss_of_t_alone_and_of_R_alone():
    d = _scene(128, 10, 0, seed=1504)
    gR, gt = _t(d["gR"]), _t(d["gt"])
    for use_R, use_t in ((False, True), (True, False)):
        p2, p3 = _t(d["pts_2d"]).requires_grad_(), _t(d["pts_3d"]).requires_grad_()
        R, t, st = pnp_batch_diff(p2, p3, _t(d["K"]))
        ((R * gR).sum() if use_R else (t * gt).sum()).backward()  # the unused output's gradient arrives as zeros
        ref = pose_vjp(R.detach(), t.detach(), st, gR if use_R else None, gt if use_t else None, pts_2d=p2.detach(), pts_3d=p3.detach(), K=_t(d["K"]))
        _sync()
        assert torch.equal(p2.grad, ref["pts_2d"]) and torch.equal(p3.grad, ref["pts_3d"]) and p2.grad.abs().max() > 0
