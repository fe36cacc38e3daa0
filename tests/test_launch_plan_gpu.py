"""The launch policy on the device: rows of tests/test_launch_plan.py (what cvxplan::plan_solve decides) against what a solve then
reports -- cvxpnpl_last_layout(), the iteration of the first certificate attempt (the smallest iteration count of the launch), and the
traces of the interior-point path.  The launch sizes are the thresholds of the policy (2 559 / 2 560, 19 999 / 20 000): the two sides of
a threshold run the same problems, and their certified poses agree as two layouts do in tests/test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import _solve, gpu  # noqa: E402,F401
from test_launch_plan import ROWS  # noqa: E402

GPU_ROWS = ("01", "02", "03", "04", "05", "08", "12", "18", "19", "28")
_DATA, _SOLVED = {}, {}


def _data(n_p, batch):
    """the first `batch` problems of ONE problem set per problem size (seed 42, 2 px noise)"""
    from cvxpnpl_amd import synth

    if n_p not in _DATA:
        _DATA[n_p] = synth.make_pnp(20000 if n_p == 10 else 2560, n_p, sigma=2.0, seed=42)
    return {k: (v[:batch] if isinstance(v, np.ndarray) and v.ndim > 2 else v) for k, v in _DATA[n_p].items()}


def _run(gpu, row):  # noqa: F811
    from cvxpnpl_amd import _lib

    if row not in _SOLVED:
        args = dict(ROWS[row][0])
        batch, n_p = args.pop("batch"), args.pop("n_p", 10)
        r = _solve(gpu, _data(n_p, batch), n_p, 0, **args)
        _SOLVED[row] = (r, _lib.lib().cvxpnpl_last_layout())
    return _SOLVED[row]


@pytest.mark.parametrize("row", GPU_ROWS)
def test_solve_runs_what_the_plan_says(gpu, row):  # noqa: F811
    args, want = ROWS[row]
    r, last_layout = _run(gpu, row)
    st, it = r["status"], r["iters"]
    print(row, "last_layout", last_layout, "iters min/max", it.min(), it.max(), "status counts", np.bincount(st, minlength=6))
    assert last_layout == want["ll"]
    assert it.min() == want["fc"]
    assert np.isin(st, (0, 1, 2, 4)).all(), np.bincount(st)  # nothing non-finite, nothing left pending
    minimal = args.get("n_p", 10) <= 4
    # as tests/test_gpu_parity.py::test_hip_vs_oracle, for the full iteration budget: minimal sets are often not tight, everything else
    # certifies.  A solve cut short (row 28: three attempts, no rescue) is held to what test_uncertified_exits_follow_reference_recovery
    # holds one to: the statuses above and the iteration cap, no certified fraction.
    if args.get("variant", 0) == 0 and "max_iters" not in args:
        assert (st == 0).mean() >= (0.5 if minimal else 0.99), np.bincount(st)
    if row in ("05", "08"):
        assert (it > 32).any()  # beyond rescue_from: the split interior-point path ran
    if row == "28":
        assert it.max() <= 7


@pytest.mark.parametrize("below,above", [("01", "02"), ("03", "04")])
def test_two_sides_of_a_threshold_agree(gpu, below, above):  # noqa: F811
    from cvxpnpl_amd import synth

    (a, la), (b, lb) = _run(gpu, below), _run(gpu, above)
    assert la != lb
    n = len(a["status"])
    assert len(b["status"]) == n + 1
    both = (a["status"] == 0) & (b["status"][:n] == 0)
    geo = synth.geodesic(a["R"], b["R"][:n])[both]
    dt = np.abs(a["t"] - b["t"][:n])[both]
    print(below, above, "certified in both", both.mean(), "geodesic max", geo.max(), "|dt| max", dt.max())
    assert both.mean() > 0.99
    assert geo.max() < 1e-7 and dt.max() < 1e-7  # (test_gpu_parity.py::test_hybrid_lane_then_wave_schedule: two layouts, both certified)
