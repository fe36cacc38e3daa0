"""The refinement kernels where the easy starts and the six shapes of tests/test_refine_gpu.py never take them: the sizes at which
cvxpnpl_refine_batch switches kernels (with masks inside every kernel), rejected trials, problems of 1 and of 100 trials in one wavefront,
max_iters of 0 to 2, scenes far from the world origin, outputs that alias the inputs, and non-finite numbers in live records.  Against the
host path of the same source, the independent reference (tests/refine_reference.py) and -- byte for byte -- against themselves.

Every batch is at most 48 problems; where the reference is slow, its rows are sampled."""
import ctypes as C

import numpy as np
import pytest
import torch

import refine_cases as rc

pytestmark = pytest.mark.gpu
FIELDS = ("R", "t", "cost", "iters", "status", "n_live", "cov")


def _dev(x, dtype=torch.float64):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda")


def _np(res):
    return type(res)(*[None if x is None else x.cpu().numpy() for x in res])


def _device(R0, t0, K, kw, status=None, **opts):
    from cvxpnpl_amd import refine as rf

    dkw = {k: _dev(v, torch.uint8 if k.startswith("mask") else torch.float64) for k, v in kw.items()}
    return _np(rf.refine_pose_batch(_dev(R0), _dev(t0), K=_dev(K), status=status, **opts, **dkw))


def _host(R0, t0, K, kw, **opts):
    from cvxpnpl_amd import refine as rf

    return rf.refine_pose_batch_host(R0, t0, K=K, **opts, **kw)


def _same_bytes(a, b, rows_a=None, rows_b=None, what=""):
    """Every output of the rows of a and of b byte for byte the same (NaN payloads included)."""
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is None:
            continue
        x = x if rows_a is None else x[rows_a]
        y = y if rows_b is None else y[rows_b]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, name)


@pytest.mark.parametrize("shape", rc.BOUNDARY_SHAPES)
def test_kernel_boundaries_with_masks(shape):
    """16, 32 and 64 correspondences are full register sets of the <1>, <2> and <4> kernels, 65 is the re-reading kernel with one record
    on a second pass, and (9, 7), (20, 12), (40, 24), (40, 25) put the point / line split inside a lane's records.  Every third record is
    masked off and spoiled (NaN / 1e9).  The same problems compacted to their live records run 11, 22, 43 and 44 records: for 65 that is
    another kernel."""
    n_p, n_l = shape
    B = 21
    d, R0, t0, kw = rc.problem(B, n_p, n_l, 1.0)
    masks = rc.boundary_masks(n_p, n_l, B)
    live = int(sum(int(m[0].sum()) for m in masks.values() if m is not None))
    spoiled = dict(rc.spoil_masked(kw, masks), **masks)
    host = _host(R0, t0, d["K"], spoiled, max_iters=100)
    dev = _device(R0, t0, d["K"], spoiled, max_iters=100)
    assert dev.status.tolist() == host.status.tolist() and (dev.status == 0).all(), (dev.status, host.status)
    assert dev.n_live.tolist() == host.n_live.tolist() == [live] * B
    assert np.isfinite(dev.R).all() and np.isfinite(dev.t).all() and np.isfinite(dev.cost).all()
    to_host = max(np.abs(dev.R - host.R).max(), np.abs(dev.t - host.t).max())
    nxt = rc.worst_next_step(d["K"], dev.R, dev.t, kw, rows=range(0, B, 4), masks=masks)
    comp = _device(R0, t0, d["K"], rc.compacted(kw, masks), max_iters=100)
    to_comp = max(np.abs(dev.R - comp.R).max(), np.abs(dev.t - comp.t).max())
    print(f"{shape}: {live} live; device to host {to_host:.1e}, to the compacted call {to_comp:.1e}, reference's next step <= {nxt:.1e}")
    assert to_host <= rc.STEP_BAR and nxt <= rc.STEP_BAR
    assert (comp.status == 0).all() and (comp.n_live == live).all() and to_comp <= rc.STEP_BAR


def test_hard_starts_on_the_device():
    """Rejected trials (lambda *= 10), trials with a record behind the camera, and the rules that end a run at the rounding floor, on the
    <1> and the <4> kernel.  Trial counts: asserted equal to the host's for at least 95 % of the problems whose reference run rejected
    nothing, over the three shapes together (29 problems: a shape alone has 9 or 10, where one differing count would already be 10 %); for
    the others the share is printed -- a rejected trial near the floor is decided by the rounding of two sums."""
    easy_same, easy_n, hard_same, hard_n = 0, 0, 0, 0
    for shape in rc.HARD_SHAPES:
        d, R0, t0, kw, runs = rc.hard_starts(shape)
        host, dev = _host(R0, t0, d["K"], kw, max_iters=100), _device(R0, t0, d["K"], kw, max_iters=100)
        assert dev.status.tolist() == host.status.tolist() and (dev.status == 0).all(), (shape, dev.status, host.status)
        cost = (np.abs(dev.cost - host.cost) / host.cost).max()
        pose = max(np.abs(dev.R - host.R).max(), np.abs(dev.t - host.t).max())
        nxt = rc.worst_next_step(d["K"], dev.R, dev.t, kw)
        print(f"{shape}: device to host, cost {cost:.1e}, pose {pose:.1e}; reference's next step <= {nxt:.1e}; trials {dev.iters.tolist()} / {host.iters.tolist()}")
        assert cost <= 1e-9 and pose <= rc.STEP_BAR and nxt <= rc.STEP_BAR
        assert (dev.cost[:, 1] <= dev.cost[:, 0]).all()
        easy = np.array([r["rejected"] == 0 for r in runs])
        same = dev.iters == host.iters
        easy_same, easy_n, hard_same, hard_n = easy_same + int(same[easy].sum()), easy_n + int(easy.sum()), hard_same + int(same[~easy].sum()), hard_n + int((~easy).sum())
    print(f"trial counts equal to the host's: {easy_same} of {easy_n} where the reference rejects nothing, {hard_same} of {hard_n} where it does")
    assert easy_same >= 0.95 * easy_n


@pytest.fixture(scope="module")
def mixed():
    """mixed_batch() once on the device: covariance, 100 trials, the statuses read from a strided column."""
    K, R0, t0, kw, expect = rc.mixed_batch()
    head = torch.zeros((12, 4), dtype=torch.int32, device="cuda")
    head[:, 1:] = 7                                              # (what a wrong stride would read: not admitted)
    return K, R0, t0, kw, expect, head, _device(R0, t0, K, kw, status=head[:, 0], max_iters=100, want_cov=True)


def test_a_problem_does_not_depend_on_its_neighbours(mixed):
    """Four problems share a wavefront and one loop; one that has ended stays frozen while the slowest of the four runs on (here: 1 trial
    and a pass-through beside 100 trials).  So every output of a problem is the same bytes alone, in the batch, and in the batch permuted."""
    K, R0, t0, kw, expect, head, full = mixed
    rc.check_mixed(full, R0, t0, expect)
    print(f"mixed batch on the device: statuses {full.status.tolist()}, trials {full.iters.tolist()}")
    assert full.iters[rc.MIXED["collinear"][0]] >= 40 and full.iters[rc.MIXED["refined"][0]] <= 2
    again = _device(R0, t0, K, kw, status=head[:, 0], max_iters=100, want_cov=True)
    _same_bytes(full, again, what="second call")
    for b in range(12):
        alone = _device(R0[b:b + 1], t0[b:b + 1], K, {k: v[b:b + 1] for k, v in kw.items() if v is not None}, status=head[b:b + 1, 0], max_iters=100,
                        want_cov=True)
        _same_bytes(full, alone, rows_a=slice(b, b + 1), what=f"problem {b} alone")
    perm = np.array([7, 3, 10, 0, 5, 8, 1, 11, 4, 2, 9, 6])     # every wavefront gets other members
    moved = _device(R0[perm], t0[perm], K, {k: v[perm] for k, v in kw.items() if v is not None}, status=head[:, 0], max_iters=100, want_cov=True)
    _same_bytes(full, moved, rows_a=perm, what="permuted")


def test_non_finite_live_data_is_status_4_and_stays_in_its_lanes(mixed):
    """NaN in a live 2D point, inf and NaN in a live 3D point: status 4, the pose passed through bit for bit, and the hard start in the same
    wavefront refined as it is on the host."""
    K, R0, t0, kw, expect, head, full = mixed
    for name in ("nan_2d", "inf_3d", "nan_3d"):
        b = rc.MIXED[name][0]
        assert 8 <= b < 12                                       # one wavefront, with the hard start at 9
        assert full.status[b] == 4 and full.iters[b] == 0 and full.n_live[b] == 10, name
        assert full.R[b].tobytes() == R0[b].tobytes() and full.t[b].tobytes() == t0[b].tobytes(), name
        assert np.isnan(full.cost[b]).all() and np.isnan(full.cov[b]).all(), name
    host = _host(R0, t0, K, kw, max_iters=100, want_cov=True)
    assert full.status[9] == host.status[9] == 0
    assert max(np.abs(full.R[9] - host.R[9]).max(), np.abs(full.t[9] - host.t[9]).max()) <= rc.STEP_BAR
    assert rc.worst_next_step(K, full.R, full.t, kw, rows=[9]) <= rc.STEP_BAR


def _scene_set():
    """Six scenes: 4, 64 and 257 points, the collinear and the coincident problem of mixed_batch(), and one whose mask leaves no live
    record.  Returns (K, [(pts_2d, pts_3d, R0, t0, mask)])."""
    scenes = []
    for i, n in enumerate((4, 64, 257)):
        d, R0, t0, kw = rc.problem(1, n, 0, 1.0, seed=40 + i)
        scenes.append((kw["pts_2d"][0], kw["pts_3d"][0], R0[0], t0[0], np.ones(n, np.uint8)))
    K, R0, t0, kw, _ = rc.mixed_batch()
    for b in (rc.MIXED["collinear"][0], rc.MIXED["coincident"][0]):
        scenes.append((kw["pts_2d"][b], kw["pts_3d"][b], R0[b], t0[b], np.ones(10, np.uint8)))
    b = rc.MIXED["ordinary"][0]
    scenes.append((kw["pts_2d"][b], kw["pts_3d"][b], R0[b], t0[b], np.zeros(10, np.uint8)))
    return K, scenes


def _run_scenes(K, scenes, **opts):
    from cvxpnpl_amd import ransac as rn, refine as rf

    sc = rn.pack_scenes([s[0] for s in scenes], [s[1] for s in scenes], K, device="cuda")
    return _np(rf.refine_scenes(sc, _dev(np.stack([s[2] for s in scenes])), _dev(np.stack([s[3] for s in scenes])),
                                mask_pts=_dev(np.concatenate([s[4] for s in scenes]), torch.uint8), max_iters=100, want_cov=True, **opts))


def test_a_scene_does_not_depend_on_the_others():
    K, scenes = _scene_set()
    full = _run_scenes(K, scenes)
    print(f"scenes: statuses {full.status.tolist()}, trials {full.iters.tolist()}, live {full.n_live.tolist()}")
    assert full.status[:3].tolist() == [0, 0, 0] and full.status[3] in (0, 1) and full.status[4:].tolist() == [3, 3]
    assert full.n_live.tolist() == [4, 64, 257, 10, 10, 0] and full.iters[4:].tolist() == [0, 0]
    for f in (4, 5):                                             # lambda ran out / nothing live: the input pose, NaN cost and covariance
        assert full.R[f].tobytes() == scenes[f][2].tobytes() and full.t[f].tobytes() == scenes[f][3].tobytes(), f
        assert np.isnan(full.cost[f]).all() and np.isnan(full.cov[f]).all(), f
    assert np.isfinite(full.R[:4]).all() and (full.cost[:4, 1] <= full.cost[:4, 0]).all() and np.isnan(full.cov[3]).all()
    _same_bytes(full, _run_scenes(K, scenes), what="second call")
    for f in range(6):
        _same_bytes(full, _run_scenes(K, scenes[f:f + 1]), rows_a=slice(f, f + 1), what=f"scene {f} alone")
    _same_bytes(full, _run_scenes(K, scenes[::-1]), rows_a=np.arange(6)[::-1], what="reversed")


@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_small_max_iters_on_the_device(max_iters):
    for shape in ((10, 0), (33, 7)):
        d, R0, t0, kw, _ = rc.hard_starts(shape)
        host, dev = _host(R0, t0, d["K"], kw, max_iters=max_iters, want_cov=True), _device(R0, t0, d["K"], kw, max_iters=max_iters, want_cov=True)
        assert dev.status.tolist() == host.status.tolist() == [1] * 12 and dev.iters.tolist() == host.iters.tolist() == [max_iters] * 12
        assert (np.abs(dev.cost - host.cost) <= 1e-9 * host.cost).all() and (dev.cost[:, 1] <= dev.cost[:, 0]).all()
        assert np.isfinite(dev.cov).all()
        if max_iters == 0:
            assert dev.R.tobytes() == R0.tobytes() and dev.t.tobytes() == t0.tobytes()            # bit for bit
            assert dev.cost[:, 0].tobytes() == dev.cost[:, 1].tobytes()


@pytest.fixture(scope="module")
def unshifted():
    d, R0, t0, kw, _ = rc.far_scene(0.0)
    return _device(R0, t0, d["K"], kw, max_iters=100, want_cov=True)


@pytest.mark.parametrize("offset", rc.FAR_OFFSETS)
def test_far_scenes_on_the_device(unshifted, offset):
    """The device's run on the shifted scene against the device's run on the unshifted one, and against the reference with the scaled h:
    the bars of tests/test_refine_hard_paths_host.py."""
    d, R0, t0, kw, o = rc.far_scene(offset)
    rc.check_far(_device(R0, t0, d["K"], kw, max_iters=100, want_cov=True), unshifted, d, kw, o, offset)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("want_cov", [False, True])
@pytest.mark.parametrize("entry", ["batch", "scenes"])
def test_outputs_may_alias_the_inputs_on_the_device(entry, want_cov):
    """include/cvxpnpl_amd_refine.h: d_R_out / d_t_out may alias the inputs.  13 problems: the three empty groups of the last wavefront
    shadow problem 12 and read its pose while its writer is about to replace it.  Pass-throughs (a NaN pose, a point behind the camera)
    sit among them: they read the input pose again when they write."""
    from cvxpnpl_amd import _lib, refine as rf

    B = 13
    d, R0, t0, kw = rc.problem(B, 8, 4, 1.0, seed=23, rot=0.5, rel_t=0.2)
    R0, t0 = R0.copy(), t0.copy()
    R0[3, 0, 0] = np.nan
    t0[6, 2] = -(kw["pts_3d"][6, 0] @ R0[6].T)[2] - 0.1
    L, o, stream = _lib.refine_lib(), rf._opts(100, 1e-10, 0.0), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p2, p3, l2, l3, K = _dev(kw["pts_2d"]), _dev(kw["pts_3d"]), _dev(kw["line_2d"]), _dev(kw["line_3d"]), _dev(d["K"])
    off_p, off_l = _dev(8 * np.arange(B + 1), torch.int64), _dev(4 * np.arange(B + 1), torch.int64)

    def call(alias):
        R, t = _dev(R0), _dev(t0)
        oR, ot, cost, iters, st, n_live, cov = rf._outputs(B, R.device, want_cov)
        if alias:
            oR, ot = R, t
        if entry == "batch":
            code = L.cvxpnpl_refine_batch(B, 8, _ptr(p2), _ptr(p3), 4, _ptr(l2), _ptr(l3), _ptr(K), 0, _ptr(R), _ptr(t), None, 1, rf.ADMIT_USABLE, None, None,
                                          C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(st), _ptr(n_live), _ptr(cov), stream)
        else:
            code = L.cvxpnpl_refine_scenes(B, _ptr(off_p), 8 * B, _ptr(off_l), 4 * B, _ptr(p2), _ptr(p3), _ptr(l2), _ptr(l3), _ptr(K), 0, _ptr(R), _ptr(t), None,
                                           1, rf.ADMIT_USABLE, None, None, C.byref(o), _ptr(oR), _ptr(ot), _ptr(cost), _ptr(iters), _ptr(st), _ptr(n_live),
                                           _ptr(cov), stream)
        assert code == 0, L.cvxpnpl_refine_last_error()
        torch.cuda.synchronize()
        return _np(rf.RefineResult(oR, ot, cost, iters, st, n_live, cov))

    fresh, in_place = call(False), call(True)
    assert fresh.status[3] == 2 and fresh.status[6] == 4 and (np.delete(fresh.status, [3, 6]) == 0).all(), fresh.status
    assert fresh.R[3].tobytes() == R0[3].tobytes() and fresh.t[6].tobytes() == t0[6].tobytes()
    _same_bytes(fresh, in_place, what=f"{entry} in place")
