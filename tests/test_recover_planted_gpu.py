"""cvxr::recover_multi_kernel (csrc/recover_kernel.h: recover_core.h compiled by hipcc, with its own fused multiply-adds)
against planted multi-pose solutions, and its launch shapes.  Reads only tests/golden/recover_planted.npz and
tests/recover_reference.py; the rules are those of tests/test_recover_planted.py (recover_reference.judge).  Every batch is
tiny for a kernel that gives one lane to a problem.
"""
import ctypes as C

import numpy as np
import pytest
import recover_reference as rr

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from cvxpnpl_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()  # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(gpu):
    from cvxpnpl_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return rr.load_fixture()


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def launch(L, gpu, status, Z, B, Q, stream=None):
    """cvxpnpl_recover_multi_device through the raw C ABI on device copies of the numpy inputs; the outputs are pre-filled with a
    sentinel.  Returns the DEVICE tensors (cnt, R, t) without synchronising."""
    import torch

    n = len(Z)
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(gpu) if a is not None else None  # noqa: E731
    st, Zd, Bd, Qd = dev(status, torch.int32), dev(Z, torch.float64), dev(B, torch.float64), dev(Q, torch.float64)
    R = torch.full((n, 4, 3, 3), SENTINEL, dtype=torch.float64, device=gpu)
    t = torch.full((n, 4, 3), SENTINEL, dtype=torch.float64, device=gpu)
    cnt = torch.full((n,), -99, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize(gpu)  # inputs and pre-fills are in place whatever stream the kernel goes to
    s = stream if stream is not None else torch.cuda.current_stream(gpu)
    rc = L.cvxpnpl_recover_multi_device(n, _p(st), _p(Zd), _p(Bd), _p(Qd), _p(R), _p(t), _p(cnt), C.c_void_p(s.cuda_stream))
    assert rc == 0, L.cvxpnpl_last_error()
    return (cnt, R, t), (st, Zd, Bd, Qd)  # the inputs stay alive until the caller has synchronised


def run(L, gpu, status, Z, B, Q):
    import torch

    (cnt, R, t), keep = launch(L, gpu, status, Z, B, Q)
    torch.cuda.synchronize(gpu)
    return cnt.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()


def host_single(L, Z55, B27, Q45=None):
    Z55, B27 = np.ascontiguousarray(Z55, dtype=np.float64), np.ascontiguousarray(B27, dtype=np.float64)
    Q45 = np.ascontiguousarray(Q45, dtype=np.float64) if Q45 is not None else None
    R, t = np.full((4, 3, 3), SENTINEL), np.full((4, 3), SENTINEL)
    n = L.cvxpnpl_recover_multi(Z55.ctypes.data_as(DP), B27.ctypes.data_as(DP), Q45.ctypes.data_as(DP) if Q45 is not None else None,
                                R.ctypes.data_as(DP), t.ctypes.data_as(DP))
    return n, R, t


# ---------------------------------------------------------------------------------------------------------- truth rules
UNPOLISHED = rr.UNPOLISHED_K2 + rr.UNPOLISHED_K4 + rr.RANK1 + rr.THRESHOLD


@pytest.fixture(scope="module")
def device_results(L, gpu, fx):
    """One launch for all classes without a cost and one for the polish classes with theirs: {class: (cnt, R, t)}."""
    out = {}
    for names, with_q in ((UNPOLISHED + rr.ODD, False), (rr.POLISHED, True)):
        Z, B, Q, who = rr.concat(names, fx)
        cnt, R, t = run(L, gpu, np.ones(len(Z), dtype=np.int32), Z, B, Q if with_q else None)
        lo = 0
        for c in names:
            n = rr.CLASSES[c][1]
            out[c] = (cnt[lo:lo + n], R[lo:lo + n], t[lo:lo + n])
            lo += n
    return out


@pytest.mark.parametrize("name", UNPOLISHED + rr.POLISHED)
def test_device_recovery_returns_the_planted_poses(device_results, fx, name):
    cnt, R, t = device_results[name]
    res = rr.judge(name, fx[name], cnt, R, t)
    print("device", rr.figures(name, res, fx[name]))


@pytest.mark.parametrize("name", rr.ODD)
def test_device_odd_and_high_ranks_are_recorded(device_results, fx, name):
    cnt, R, t = device_results[name]
    found = rr.check_odd(name, fx[name], cnt, R, t)
    print(f"device {name}: {found} of {fx[name]['R'].shape[0] * fx[name]['R'].shape[1]} planted poses found")


def test_device_reflection_is_left_unpolished_and_finite(L, gpu, fx):
    """A candidate with det R < 0 (a rank-1 Z planted from an improper orthogonal matrix) next to a proper one, with a generic
    cost that is no null-space cost: the reflection comes back finite and bit for bit as without a cost, the proper one is moved."""
    rs = np.random.RandomState(5)
    M = rs.normal(size=(9, 12))
    q45 = rr.pack_q45(M @ M.T)
    proper = fx["r1_exact"]["R"][0, 0]
    improper = proper @ np.diag([1.0, 1.0, -1.0])
    Z = np.stack([rr.vech10(rr.plant_Z([improper], [1.0])), rr.vech10(rr.plant_Z([proper], [1.0]))])
    B = np.stack([fx["r1_exact"]["B27"][0]] * 2)
    ones = np.ones(2, dtype=np.int32)
    c0, R0, t0 = run(L, gpu, ones, Z, B, None)
    c1, R1, t1 = run(L, gpu, ones, Z, B, np.stack([q45, q45]))
    assert (c0 == 1).all() and (c1 == 1).all() and np.linalg.det(R0[0, 0]) < 0
    assert np.isfinite(R1[:, 0]).all() and np.isfinite(t1[:, 0]).all()
    assert np.array_equal(R0[0], R1[0], equal_nan=True) and np.array_equal(t0[0], t1[0], equal_nan=True)
    assert np.abs(R0[0, 0] - improper).max() < 1e-14
    assert np.abs(R1[1, 0] - proper).max() > 1e-3 and np.abs(R1[1, 0] @ R1[1, 0].T - np.eye(3)).max() < 1e-14


def test_planar_twins_give_both_poses_and_no_nan(device_results, fx):
    """The exact two-fold ambiguity: equal eigenvalues, an arbitrary basis of the eigenspace, the top eigenvector's last entry can
    be ~0 -- the reference returns NaN on a good part of these.  128 problems: two poses each, both planted ones, nothing NaN."""
    total = 0
    for name in ("planar_eq", "planar_73"):
        cnt, R, t = device_results[name]
        assert (cnt == 2).all() and np.isfinite(R[:, :2]).all() and np.isfinite(t[:, :2]).all(), name
        for i in range(len(cnt)):
            err, match = rr.rot_err(R[i, :2], fx[name]["R"][i])
            assert err <= rr.FLOOR and sorted(match) == [0, 1], (name, i, err)
        total += len(cnt)
    assert total == 128


# --------------------------------------------------------------------------------------------------------- launch shape
# neighbours in a wavefront: rank 1, k = 2, k = 4, a planar twin, a threshold member, ...
SHAPE_CLASSES = ("r1_exact", "k2_rand_w02", "k4_rand_w25", "planar_eq", "thr_lo", "k4_near", "k2_twin_01", "thr_hi", "r1_pert", "k4_rand_w02", "planar_73")
STATUS_DEAL = (1, 1, 0, 1, 2, 1, 3, 1, 4)  # RANK_GT1 and every status that is skipped; 9 and 7 (NaN) and 11 (classes) are coprime


def shaped_batch(fx, n):
    """n problems dealt from SHAPE_CLASSES in turn; statuses dealt from STATUS_DEAL (a batch of one is flagged); Z of every 7th
    problem NaN.  Returns Z, B, status and (class, index) per problem."""
    who = [(SHAPE_CLASSES[i % len(SHAPE_CLASSES)], (i // len(SHAPE_CLASSES)) % rr.CLASSES[SHAPE_CLASSES[i % len(SHAPE_CLASSES)]][1]) for i in range(n)]
    Z = np.stack([fx[c]["Z55"][j] for c, j in who])
    B = np.stack([fx[c]["B27"][j] for c, j in who])
    status = np.array([STATUS_DEAL[i % 9] for i in range(n)], dtype=np.int32) if n > 1 else np.ones(1, dtype=np.int32)
    nan = np.zeros(n, dtype=bool)
    nan[3::7] = True
    Z[nan] = np.nan
    return Z, B, status, who, nan


def pair_bound(fx, c, j):
    """Device against host on one problem: the bound of the truth rules where the class has one, the floor otherwise (rank 1)."""
    if c in rr.UNPOLISHED_K2 + rr.UNPOLISHED_K4 + ("r1_exact", "thr_hi"):  # r1_pert, thr_lo: rank 1, no conditioning to allow for
        return rr.bound_unpolished(fx[c]["ref_err"][j], 4 if c in rr.UNPOLISHED_K4 else 2)
    return rr.FLOOR


@pytest.fixture(scope="module")
def host_cache(L, fx):
    cache = {}

    def get(c, j):
        if (c, j) not in cache:
            cache[(c, j)] = host_single(L, fx[c]["Z55"][j], fx[c]["B27"][j])
        return cache[(c, j)]

    return get


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129, 4097))
def test_launch_shapes_against_single_host_calls(L, gpu, fx, host_cache, n):
    Z, B, status, who, nan = shaped_batch(fx, n)
    if n >= 64:  # every full wavefront mixes flagged, each kind of unflagged, and NaN lanes
        for w in range(n // 64):
            s = slice(64 * w, 64 * w + 64)
            assert set(status[s]) == {0, 1, 2, 3, 4} and (nan[s] & (status[s] == 1)).any() and (~nan[s] & (status[s] == 1)).any()
    assert n % 64 != 0 or n == 64  # the last block is partial (64 itself: the full-block edge)
    cnt, R, t = run(L, gpu, status, Z, B, None)
    worst = 0.0
    for i, (c, j) in enumerate(who):
        if status[i] != 1:
            assert cnt[i] == 0 and np.isnan(R[i]).all() and np.isnan(t[i]).all(), (i, c, j, "skipped")
            continue
        if nan[i]:
            assert cnt[i] == -1 and np.isnan(R[i]).all() and np.isnan(t[i]).all(), (i, c, j, "NaN Z")
            continue
        nh, Rh, th = host_cache(c, j)
        assert cnt[i] == nh, (i, c, j, int(cnt[i]), nh)
        assert np.isnan(R[i, nh:]).all() and np.isnan(t[i, nh:]).all(), (i, c, j)
        bound = pair_bound(fx, c, j)
        scale = max(1.0, np.abs(fx[c]["B27"][j].reshape(3, 9)).sum(axis=1).max())
        e1, m1 = rr.rot_err(R[i, :nh], Rh[:nh])   # every host pose has a device pose
        e2, m2 = rr.rot_err(Rh[:nh], R[i, :nh])   # and the other way round
        et = max(np.abs(t[i, m1[k]] - th[k]).max() for k in range(nh)) / scale
        worst = max(worst, max(e1, e2, et) / bound)
        assert max(e1, e2, et) <= bound, (i, c, j, e1, e2, et, bound)
    print(f"batch {n}: worst device-host distance / bound = {worst:.2e}")


def test_nan_neighbour_changes_nothing(L, gpu, fx):
    Z, B, status, who, nan = shaped_batch(fx, 65)
    clean = np.stack([fx[c]["Z55"][j] for c, j in who])
    a = run(L, gpu, status, Z, B, None)
    b = run(L, gpu, status, clean, B, None)
    keep = ~nan
    for x, y in zip(a, b):
        assert np.array_equal(x[keep], y[keep], equal_nan=True)
    assert (a[0][nan & (status == 1)] == -1).all() and (b[0][nan & (status == 1)] > 0).all()


# ------------------------------------------------------------------------------------------------------- null arguments
def test_null_status_recovers_every_problem(L, gpu, fx):
    Z, B, status, who, nan = shaped_batch(fx, 129)
    cnt, R, t = run(L, gpu, None, Z, B, None)
    ones = run(L, gpu, np.ones(129, dtype=np.int32), Z, B, None)
    assert (cnt != 0).all() and (cnt[nan] == -1).all() and (cnt[~nan] > 0).all()
    assert not (R == SENTINEL).any() and not (t == SENTINEL).any()
    for x, y in zip((cnt, R, t), ones):
        assert np.array_equal(x, y, equal_nan=True)


def test_back_to_back_calls_with_and_without_cost_on_a_side_stream(L, gpu, fx):
    """Q45 == NULL and Q45 present, one after the other on a side stream with nothing between them: each gives what it gives
    alone; two identical calls are bit-identical."""
    import torch

    Z, B, Q, who = rr.concat(rr.POLISHED, fx)
    status = np.ones(len(Z), dtype=np.int32)
    alone_plain = run(L, gpu, status, Z, B, None)
    alone_cost = run(L, gpu, status, Z, B, Q)
    again = run(L, gpu, status, Z, B, Q)
    for x, y in zip(alone_cost, again):
        assert np.array_equal(x, y, equal_nan=True)
    side = torch.cuda.Stream(device=gpu)
    out1, keep1 = launch(L, gpu, status, Z, B, None, stream=side)
    out2, keep2 = launch(L, gpu, status, Z, B, Q, stream=side)
    side.synchronize()
    for x, y in zip(out1, alone_plain):
        assert np.array_equal(x.cpu().numpy(), y, equal_nan=True)
    for x, y in zip(out2, alone_cost):
        assert np.array_equal(x.cpu().numpy(), y, equal_nan=True)
    assert not np.array_equal(alone_plain[1], alone_cost[1], equal_nan=True)  # the noise classes: the polish moved them


def test_empty_batch_and_null_pointers(L, gpu, fx):
    import torch

    Z, B, status, who, nan = shaped_batch(fx, 4)
    (cnt, R, t), (st, Zd, Bd, Qd) = launch(L, gpu, status, Z, B, None)
    torch.cuda.synchronize(gpu)
    s = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert L.cvxpnpl_recover_multi_device(0, _p(st), _p(Zd), _p(Bd), None, _p(R), _p(t), _p(cnt), s) == 0
    for args in ((4, _p(st), None, _p(Bd), None, _p(R), _p(t), _p(cnt), s),
                 (4, _p(st), _p(Zd), None, None, _p(R), _p(t), _p(cnt), s),
                 (4, _p(st), _p(Zd), _p(Bd), None, None, _p(t), _p(cnt), s),
                 (4, _p(st), _p(Zd), _p(Bd), None, _p(R), None, _p(cnt), s),
                 (4, _p(st), _p(Zd), _p(Bd), None, _p(R), _p(t), None, s),
                 (-1, _p(st), _p(Zd), _p(Bd), None, _p(R), _p(t), _p(cnt), s)):
        assert L.cvxpnpl_recover_multi_device(*args) == -1
        assert b"cvxpnpl_recover_multi_device: bad arguments" in L.cvxpnpl_last_error()
    torch.cuda.synchronize(gpu)
