"""The launch policy of a solve (csrc/launch_plan.h: cvxplan::validate / plan_solve) on the host, without a GPU: which kernel runs first,
with which grid, hand-off point and attempt schedule, which workspace it needs and which launches follow -- for every threshold and
every request the policy rewrites.  The header is built with g++ into tests/hostsim/libplanshim.so (plan_shim.cpp).
tests/test_launch_plan_gpu.py holds a subset of the same rows against what the device then reports."""
import ctypes as C
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RS_LANE, RS_FULL, MAXR, MAXI, WPB = 56, 240, 2048, 2048, 1  # cvxw::RS_LANE, RS_FULL, RESUME_GRID_MAX, cvxi::IPMQ_GRID_MAX, cvxw::WPB
AUTO, LANE, WAVE, QUAD, PENTA = 0, 1, 2, 3, 4  # CVXPNPL_LAYOUT_*
KERNELS = ("wave_full", "wave_rc", "lane2_f32", "lane2_f64", "quad", "quad_f64", "quad_penta", "quad_rc", "quad_rc_f64", "quad_minimal",
           "quad_minimal_f64")  # cvxplan::FirstKernel
RESUME, IPM, RESCUE = 0, 1, 2  # cvxplan::FollowKind
MAX_FOLLOW = 4


class PlanFlat(C.Structure):
    _fields_ = [("valid", C.c_int32), ("too_large", C.c_int32), ("layout", C.c_int32), ("last_layout", C.c_int32), ("handoff_at", C.c_int32),
                ("first", C.c_int32), ("first_grid", C.c_int64), ("first_check", C.c_int32), ("rescue_from", C.c_int32),
                ("f32_sweeps_until", C.c_int32), ("dual_shift", C.c_double), ("rescue", C.c_int32), ("split", C.c_int32), ("ws_stride", C.c_int32),
                ("needs_workspace", C.c_int32), ("n_follow", C.c_int32), ("kind", C.c_int32 * MAX_FOLLOW), ("stride", C.c_int32 * MAX_FOLLOW),
                ("full", C.c_int32 * MAX_FOLLOW), ("two_queues", C.c_int32 * MAX_FOLLOW), ("grid", C.c_int64 * MAX_FOLLOW), ("err", C.c_char * 256)]


def _opts(**kw):
    import hostsim
    from cvxpnpl_amd._lib import Opts

    o = Opts()
    hostsim.plan_lib().plan_default_opts(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def plan(batch, n_p=10, n_l=0, cost_seam=False, null_opts=False, **kw):
    import hostsim

    L = hostsim.plan_lib()
    out = PlanFlat()
    lim = (C.c_int32 * 5)(RS_LANE, RS_FULL, MAXR, MAXI, WPB)
    o = None if null_opts else _opts(**kw)
    L.plan_flat(C.c_int64(batch), C.c_int32(n_p), C.c_int32(n_l), C.c_int32(int(cost_seam)), C.byref(o) if o is not None else None, lim, C.byref(out))
    return out


def follow(p):
    """[(kind, grid, stride, full, two_queues)] of a plan"""
    return [(p.kind[i], p.grid[i], p.stride[i], bool(p.full[i]), bool(p.two_queues[i])) for i in range(p.n_follow)]


def rgrid(b):
    return min(b, MAXR)


def ipm_then_resume_full(b):  # the split interior-point path behind a quad phase: two rounds
    return 2 * [(IPM, min(math.ceil(b / 4), MAXI), RS_FULL, True, False), (RESUME, rgrid(b), RS_FULL, True, False)]


def ipm_then_resume_lane(b):  # ... behind a wave kernel
    return [(IPM, min(math.ceil(b / 4), MAXI), RS_LANE, False, False), (RESUME, rgrid(b), RS_LANE, False, False)]


def rescue_one(b):
    return [(RESCUE, rgrid(b), RS_FULL, True, False)]


def rescue_two(b):
    return [(RESCUE, 2 * rgrid(b), RS_FULL, True, True)]


def resume_full(b):
    return [(RESUME, rgrid(b), RS_FULL, True, False)]


# id -> (arguments of plan(), expectations).  Expectations: ll = cvxpnpl_last_layout(), k = first kernel, grid, ho = hand-off point
# (0: the wave kernel runs the whole solve), fc = resolved first_check, rf = resolved rescue_from, rescue / split, ws = workspace
# stride, needs_ws, follow = the launches behind the first kernel.  A key that is absent is not stated for that row.
ROWS = {
    "01": (dict(batch=2559), dict(ll=WAVE, k="wave_full", grid=2559, ho=0, fc=5, rf=128, rescue=True, split=False, ws=0, needs_ws=True, follow=rescue_one(2559))),
    "02": (dict(batch=2560), dict(ll=QUAD, k="quad", grid=640, ho=7, fc=5, rf=128, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(2560))),
    "03": (dict(batch=19999), dict(ll=QUAD, k="quad", grid=5000, ho=7, fc=5, rf=128, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(19999))),
    "04": (dict(batch=20000), dict(ll=LANE, k="lane2_f32", grid=313, ho=6, fc=6, rf=128, rescue=True, split=False, ws=RS_LANE,
                                   follow=[(RESUME, MAXR, RS_LANE, False, False)] + rescue_one(20000))),
    "05": (dict(batch=2560, n_p=4), dict(ll=QUAD, k="quad_minimal", grid=640, ho=24, fc=17, rf=32, rescue=True, split=True, ws=RS_FULL, follow=ipm_then_resume_full(2560))),
    "06": (dict(batch=30000, n_p=4), dict(ll=QUAD, k="quad_minimal", grid=7500, ho=24, fc=17, rf=32, rescue=True, split=True, ws=RS_FULL, follow=ipm_then_resume_full(30000))),
    "07": (dict(batch=2560, n_p=4, f32_sweeps_until=0), dict(ll=QUAD, k="quad_minimal_f64", grid=640, ho=24, fc=17, rf=32, split=True, ws=RS_FULL, follow=ipm_then_resume_full(2560))),
    "08": (dict(batch=2559, n_p=4), dict(ll=WAVE, k="wave_full", grid=2559, ho=0, fc=5, rf=32, rescue=True, split=True, ws=RS_LANE, follow=ipm_then_resume_lane(2559))),
    "09": (dict(batch=2560, n_p=4, layout=QUAD), dict(ll=QUAD, k="quad", grid=640, ho=7, fc=5, rf=32, split=True, ws=RS_FULL, follow=ipm_then_resume_full(2560))),
    "10": (dict(batch=2560, n_p=4, lane_iters=10), dict(ll=QUAD, k="quad", ho=10, fc=5, rf=32, split=True, ws=RS_FULL, follow=ipm_then_resume_full(2560))),
    "11-n5": (dict(batch=10000, n_p=5), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=32, rescue=True, split=True, ws=RS_FULL)),
    "11-n6": (dict(batch=10000, n_p=6), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=32, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(10000))),
    "11-n7": (dict(batch=10000, n_p=7), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=64, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(10000))),
    "11-n8": (dict(batch=10000, n_p=8), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=128, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(10000))),
    "12": (dict(batch=10000, variant=1), dict(ll=QUAD, k="quad_rc", grid=2500, ho=36, fc=19, rf=48, rescue=True, split=True, ws=RS_FULL, follow=ipm_then_resume_full(10000))),
    "13": (dict(batch=30000, variant=1), dict(ll=QUAD, k="quad_rc", grid=7500, ho=36, fc=19, rf=48, rescue=True, split=True, ws=RS_FULL)),
    "14": (dict(batch=1000, variant=1), dict(ll=WAVE, k="wave_rc", grid=1000, ho=0, fc=11, rf=48, rescue=True, split=True, ws=RS_LANE, follow=ipm_then_resume_lane(1000))),
    "15": (dict(batch=10000, variant=1, f32_sweeps_until=0), dict(ll=QUAD, k="quad_rc_f64", ho=36, fc=19, rf=48, split=True, ws=RS_FULL)),
    "16": (dict(batch=10000, variant=1, lane_iters=60), dict(ll=QUAD, k="quad_rc", ho=48, fc=19)),
    "17": (dict(batch=10000, layout=QUAD, lane_iters=40), dict(ll=QUAD, k="quad", ho=16, fc=5)),
    "18": (dict(batch=10000, layout=PENTA), dict(ll=PENTA, k="quad_penta", grid=2000, ho=7, fc=5, rf=128, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(10000))),
    "19": (dict(batch=10000, layout=PENTA, f32_sweeps_until=0), dict(ll=QUAD, k="quad_f64", grid=2500, ho=7, fc=5, ws=RS_FULL, follow=rescue_two(10000))),
    "20": (dict(batch=10000, variant=1, layout=PENTA), dict(ll=QUAD, k="quad_rc", ho=36, fc=19)),
    "21": (dict(batch=30000, layout=LANE, lane_iters=4), dict(ll=QUAD, k="quad", ho=7, fc=5, ws=RS_FULL, follow=rescue_two(30000))),
    "22": (dict(batch=30000, layout=LANE, warm_start=0), dict(ll=QUAD, k="quad", ho=7, fc=5)),
    "23": (dict(batch=1000, layout=LANE, lane_iters=4), dict(ll=WAVE, k="wave_full", ho=0, fc=5, follow=rescue_one(1000))),
    "24": (dict(batch=30000, layout=LANE, lane_iters=4, first_check=4), dict(ll=LANE, k="lane2_f32", ho=4, fc=4, ws=RS_LANE)),
    "25": (dict(batch=30000, layout=LANE, first_check=8), dict(ll=QUAD, k="quad", ho=7, fc=8)),  # (8 != the lane phase's cap of 6)
    "26": (dict(batch=30000, f32_sweeps_until=0), dict(ll=LANE, k="lane2_f64", ho=6, fc=6)),
    "27-f32": (dict(batch=30000, f32_sweeps_until=6), dict(ll=LANE, k="lane2_f32", ho=6, fc=6)),
    "27-f64": (dict(batch=30000, f32_sweeps_until=5), dict(ll=LANE, k="lane2_f64", ho=6, fc=6)),
    "28": (dict(batch=10000, max_iters=7), dict(ll=WAVE, k="wave_full", grid=10000, ho=0, fc=5, rf=128, rescue=False, ws=0, needs_ws=False, follow=[])),  # (7 > 7 is false)
    "29": (dict(batch=10000, max_iters=8), dict(ll=QUAD, k="quad", ho=7, fc=5, rescue=False, ws=RS_FULL, follow=resume_full(10000))),
    "30": (dict(batch=30000, max_iters=6), dict(ll=LANE, k="wave_full", grid=30000, ho=0, fc=6, rescue=False, ws=0, needs_ws=False, follow=[])),  # (no hybrid)
    "31": (dict(batch=10000, n_p=0, cost_seam=True), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=128, rescue=True, split=False, ws=RS_FULL, follow=rescue_two(10000))),
    "32": (dict(batch=10000, rescue_from=0), dict(ll=QUAD, k="quad", ho=7, fc=5, rf=0, rescue=False, ws=RS_FULL, follow=resume_full(10000))),
    "33-f32": (dict(batch=10000, f32_sweeps_until=7), dict(ll=QUAD, k="quad", ho=7, fc=5)),
    "33-f64": (dict(batch=10000, f32_sweeps_until=6), dict(ll=QUAD, k="quad_f64", ho=7, fc=5)),
    "34": (dict(batch=10000, n_p=3, n_l=1), dict(ll=QUAD, k="quad_minimal", grid=2500, ho=24, fc=17, rf=32, split=True, follow=ipm_then_resume_full(10000))),
    "35": (dict(batch=10000, null_opts=True), dict(ll=QUAD, k="quad", grid=2500, ho=7, fc=5, rf=128, dual_shift=0.015, follow=rescue_two(10000))),
}
FIELD = {"ll": "last_layout", "grid": "first_grid", "ho": "handoff_at", "fc": "first_check", "rf": "rescue_from", "ws": "ws_stride",
         "needs_ws": "needs_workspace", "rescue": "rescue", "split": "split", "dual_shift": "dual_shift"}


@pytest.mark.parametrize("row", sorted(ROWS))
def test_plan_row(row):
    args, want = ROWS[row]
    p = plan(**args)
    assert p.valid and not p.too_large, p.err
    got = {"k": KERNELS[p.first], "follow": follow(p)}
    got.update({k: getattr(p, f) for k, f in FIELD.items()})
    for k, v in want.items():
        assert got[k] == v, (row, k, got[k], v)
    # what holds for every plan: a parked iterate needs a workspace of its stride, and the quad schedule always parks
    assert p.needs_workspace or (p.ws_stride == 0 and p.n_follow == 0)
    assert (p.ws_stride == RS_FULL) == (p.layout == QUAD) and p.n_follow <= MAX_FOLLOW
    if p.rescue and not p.split:  # the fused interior-point path: one launch, behind everything else
        assert follow(p)[-1:] == (rescue_two if p.layout == QUAD else rescue_one)(args["batch"])


def test_dual_shift_by_variant():
    assert plan(10000, variant=1).dual_shift == 0.006
    assert plan(10000).dual_shift == 0.015  # cvx::DUAL_SHIFT_DEFAULT
    assert plan(10000, variant=1, dual_shift=0.25).dual_shift == 0.25


BAD = [dict(max_iters=0), dict(f32_sweeps_until=-2), dict(f32_sweeps_until=65), dict(rho=0.0), dict(rho=float("nan")), dict(eps=0.0), dict(eps=float("nan")),
       dict(check_every=0), dict(first_check=-1), dict(variant=2), dict(variant=-1), dict(adapt_every=-1), dict(adapt_every=10, adapt_mu=0.5),
       dict(adapt_every=10, adapt_tau=1.0), dict(rescue_from=-2), dict(dual_shift=1.5), dict(dual_shift=-0.5), dict(dual_refine=-2), dict(dual_refine=2)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_options_are_refused(kw):
    p = plan(10000, **kw)
    assert not p.valid and p.err == b"cvxpnpl: bad options"


@pytest.mark.parametrize("layout", [5, 9, -1])
def test_unknown_layout_is_refused(layout):
    p = plan(10000, layout=layout)
    assert not p.valid and p.err == f"cvxpnpl: bad options (layout {layout} is not one of CVXPNPL_LAYOUT_*)".encode()


def test_wrong_struct_size_is_refused():
    from cvxpnpl_amd._lib import Opts

    size = C.sizeof(Opts)
    p = plan(10000, struct_size=size - 8)
    assert not p.valid
    assert p.err == (f"cvxpnpl: options block of {size - 8} bytes, this library's cvxpnpl_opts_t has {size} "
                     "(cvxpnpl_default_opts / cvxpnpl_opts_size)").encode()


def test_options_the_policy_accepts():
    """the edges of the validation on the accepting side, and the defaults themselves"""
    for kw in (dict(), dict(f32_sweeps_until=64), dict(f32_sweeps_until=-1), dict(adapt_every=0, adapt_mu=0.0), dict(rescue_from=-1), dict(dual_shift=0.0),
               dict(dual_shift=1.0), dict(dual_refine=-1), dict(dual_refine=1), dict(layout=PENTA)):
        assert plan(10000, **kw).valid, kw
    assert plan(10000, null_opts=True).valid


def test_batch_too_large_for_one_launch():
    assert plan(2 ** 31, layout=WAVE).too_large  # one block per problem
    assert not plan(2 ** 31 - 1, layout=WAVE).too_large
    assert plan(2 ** 37 + 1, layout=QUAD).too_large and not plan(2 ** 32, layout=QUAD).too_large
