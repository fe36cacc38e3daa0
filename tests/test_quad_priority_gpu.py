"""The quad kernel's issue priorities (cvxq::solve_quad_kernel: s_setprio for second-round blocks and for wavefronts with an open problem
after a certificate attempt, quad_kernel.h) change who wins the VALU slot of a SIMD and nothing else.  What they could disturb is timing:
which wavefront reaches the queue of planar scenes first, when a wavefront reads back the iterate it parked for itself.  So: one batch that
mixes ordinary, planar and non-finite problems, larger than one round of the chip's wavefront slots (2 048 x 4 problems), in the quad layout
against the wave layout -- to the tolerances tests/test_gpu_parity.py uses between these layouts (test_hybrid_lane_then_wave_schedule,
test_hybrid_queue_counters_alternate_between_launches) -- and twice in a row, which must give the same answer bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QUAD, WAVE = 3, 2  # CVXPNPL_LAYOUT_*
N_PTS = 10
BATCH = 12000  # 3 000 wavefronts: 952 of them start behind the first round


@pytest.fixture(scope="module")
def gpu():
    import torch

    from cvxpnpl_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def _mixed_batch():
    from cvxpnpl_amd import synth

    plain = synth.make_pnp(BATCH, N_PTS, 2.0, seed=71)
    planar = synth.make_planar_pnp(BATCH, N_PTS, 0.5, seed=72, general=True)
    i = np.arange(BATCH)
    is_planar = i % 7 == 3
    is_nonfinite = (i % 11 == 5) & ~is_planar
    d = {k: plain[k].copy() for k in ("pts_2d", "pts_3d")}
    for k in d:
        d[k][is_planar] = planar[k][is_planar]
    d["pts_2d"][is_nonfinite, 0, 0] = np.nan
    d["pts_3d"][is_nonfinite & (i % 2 == 0), 1, 2] = np.inf
    d["K"] = plain["K"]
    return d, is_planar, is_nonfinite


def _solve(gpu, d, **kw):
    import torch

    import cvxpnpl_amd as ca

    res = ca.pnp_batch(torch.as_tensor(d["pts_2d"], device=gpu), torch.as_tensor(d["pts_3d"], device=gpu), torch.as_tensor(d["K"], device=gpu), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("f64_sweeps", [True, False])
def test_mixed_batch_quad_equals_wave(gpu, f64_sweeps):
    from cvxpnpl_amd import synth

    d, is_planar, is_nonfinite = _mixed_batch()
    kw = {"max_iters": 300}
    if f64_sweeps:
        kw["f32_sweeps_until"] = 0  # cvxq::solve_quad_kernel<0, 2, 16, true, 0>, the kernel of bench.py's default run
    w = _solve(gpu, d, layout=WAVE, **kw)
    q1 = _solve(gpu, d, layout=QUAD, **kw)
    q2 = _solve(gpu, d, layout=QUAD, **kw)
    # the same launch twice: the same answer, bit for bit
    for k in ("status", "iters"):
        assert np.array_equal(q1[k], q2[k]), k
    for k in ("R", "t"):
        assert np.array_equal(q1[k], q2[k], equal_nan=True), k
    for r in (w, q1):
        assert np.isin(r["status"], (0, 1, 2, 3, 4)).all(), np.unique(r["status"])  # nothing left pending on a queue
        assert (r["status"][is_nonfinite] == 3).all()
        assert np.isnan(r["R"][is_nonfinite]).all() and np.isnan(r["t"][is_nonfinite]).all()
        assert (r["status"][~is_nonfinite] != 3).all()
    same = q1["status"] == w["status"]
    assert same.mean() > 0.995, same.mean()
    both = same & (q1["status"] == 0)
    assert both.sum() > 0.8 * (~is_planar & ~is_nonfinite).sum()
    assert synth.geodesic(q1["R"], w["R"])[both].max() < 1e-7
    assert np.abs(q1["t"] - w["t"])[both].max() < 1e-7
    assert np.median(synth.geodesic(q1["R"], w["R"])[both]) < 1e-14
    fl = same & (q1["status"] == 1)  # rank > 1 (the planar scenes): a certified twin pair, or the NaN rounding at the iteration cap -- like the wave layout
    assert fl.any()
    assert (np.isnan(q1["R"][fl]).any(axis=(1, 2)) == np.isnan(w["R"][fl]).any(axis=(1, 2))).mean() > 0.995
