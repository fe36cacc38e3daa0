"""The library of local optimisation in adaptive RANSAC (libcvxpnpl_amd_ransac_lo.so, include/cvxpnpl_amd_ransac_lo.h; DESIGN.md section
24): it builds by cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device,
keeps its kernels free of scratch and spills (tests/golden/ransac_lo_kernel_resources.json), leaves the other thirteen libraries alone
and lists its dependencies exactly; its assembly rule on the host against the numpy reference's predicate (tests/ransac_lo_reference.py)
and the host build's assembly of the gathered set; the host-side validation of ransac_pnp_batch(local_opt=, lo_widen=); the reference's
replay on hand-made numbers; and the experiment that motivates it, on the host build of the device algorithm.  No GPU needed."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_lo_reference import SceneReplay, pack45, simulate_lo, take_fit, taken, widen
from ransac_msac_reference import perturbed_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_lo_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxnlo::lo_assemble_active_kernel", "cvxnlo::lo_update_active_kernel", "cvxnlo::lo_init_kernel")
MARGIN = 1e-9        # every |r^2 - tau^2| / tau^2 of the inputs is above this at every threshold used, so that the taken set is unambiguous
THRESH = 2.0
WIDEN = (1.0, 1.5, 2.0)
SIZES = (4, 63, 64, 65, 512, 513, 700)


def make_case(sizes, seed=5, per_scene_K=False, thresholds=tuple(THRESH * m for m in WIDEN), outliers=None):
    """Scenes of synth.make_ransac (30 % clutter unless `outliers` gives a share per scene, 1 px noise) of the given sizes with one
    RUNNING pose per scene a little off the ground truth (up to 0.1 degrees, 0.2 % of |t|), so that the sets taken at the thresholds
    differ.  The seed is redrawn until no residual sits within MARGIN of any threshold.  Returns a dict of numpy arrays: x [sum M,2],
    X [sum M,3], sizes, off, K, R [F,3,3], t [F,3], R_gt, t_gt, and masks {threshold: packed bool [sum M]} by the reference's predicate."""
    from cvxpnpl_amd import synth

    for attempt in range(8):
        rs = np.random.RandomState(seed + 1000 * attempt)
        xs, Xs, Rs, ts, Ks, Rg, tg = [], [], [], [], [], [], []
        for f, m in enumerate(sizes):
            K = np.array(synth.K_KINECT, dtype=np.float64)
            if per_scene_K:
                K[0, 0] *= 1.0 + 0.02 * f
                K[1, 1] *= 1.0 - 0.02 * f
            d = synth.make_ransac(1, n_corr=m, outlier_frac=0.3 if outliers is None else outliers[f], sigma=1.0, seed=seed + 1000 * attempt + f, K=K)
            R, t = perturbed_poses(d["R_gt"], d["t_gt"], 2, rs, max_deg=0.1, max_rel=0.002)
            xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); Rs.append(R[1]); ts.append(t[1]); Ks.append(K); Rg.append(d["R_gt"]); tg.append(d["t_gt"])
        off = np.concatenate([[0], np.cumsum(sizes)])
        case = {"x": np.concatenate(xs), "X": np.concatenate(Xs), "sizes": list(sizes), "off": off, "K": np.stack(Ks) if per_scene_K else Ks[0],
                "R": np.stack(Rs), "t": np.stack(ts), "R_gt": np.stack(Rg), "t_gt": np.stack(tg), "masks": {}}
        margin = np.inf
        for th in thresholds:
            mk, m = reference_masks(case, case["R"], case["t"], th)
            case["masks"][th], margin = mk, min(margin, m)
        if margin > MARGIN:
            case["margin"] = margin
            return case
    raise AssertionError("no seed keeps every residual away from the thresholds")


def scene_K(case, f):
    return case["K"][f] if np.ndim(case["K"]) == 3 else case["K"]


def reference_masks(case, R, t, thresh):
    """packed mask of the poses (R, t)[f] over the scenes of a case, by the reference's predicate, and the least margin"""
    off, mk, margin = case["off"], np.zeros(len(case["x"]), dtype=bool), np.inf
    for f in range(len(case["sizes"])):
        s = slice(off[f], off[f + 1])
        mk[s], m = taken(case["x"][s], case["X"][s], scene_K(case, f), R[f], t[f], thresh)
        margin = min(margin, m)
    return mk, margin


def assert_cost_close(B, Q, B_ref, Q_ref, who):
    """the project's own assembly tolerance (tests/test_ransac_batch_gpu.py): the summation order differs, so no bit-equality"""
    B, Q, B_ref, Q_ref = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (B, Q, B_ref, Q_ref))
    assert np.isfinite(B).all() and np.isfinite(Q).all(), who
    assert np.max(np.abs(Q - Q_ref)) <= 1e-11 * np.max(np.abs(Q_ref)), (who, np.max(np.abs(Q - Q_ref)), np.max(np.abs(Q_ref)))
    assert np.max(np.abs(B - B_ref)) <= 1e-9 * max(1.0, np.max(np.abs(B_ref))), (who, np.max(np.abs(B - B_ref)))


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_lo()
    assert os.path.exists(build.RANSAC_LO_OUT)
    return _lib.ransac_lo_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_lo.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_LO_EXPORTS), declared ^ set(_lib.RANSAC_LO_EXPORTS)
    assert all(name.startswith("cvxpnpl_ransac_lo_") for name in declared)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_LO_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library_and_exact_dependencies():
    """The fourteenth pair is named apart from the twelve tests/test_build_deps.py pins; the property it checks is checked here."""
    from test_build_deps import include_closure

    from cvxpnpl_amd import build as b

    assert b.ransac_lo_command("x")[:-1] == b.ransac_compile_cmd("x")[:-1]
    sources = [c for c in b.ransac_lo_command("x") if c.endswith((".hip", ".cpp"))]
    assert sources == [b.RANSAC_LO_SRC]
    listed = [os.path.realpath(d) for d in b.RANSAC_LO_SOURCES]
    assert len(listed) == len(set(listed))
    closure = include_closure(sources)
    assert set(listed) == closure, (sorted(closure - set(listed)), sorted(set(listed) - closure))


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_lo_last_error
    nan, z = float("nan"), None

    def named(call, names, **fixed):
        for name, word in names.items():
            assert call(**{name: None}, **fixed) == -1, name
            assert word.encode() in err(), (name, err())

    def init(F=2, taken_=p):
        return G.cvxpnpl_ransac_lo_init(F, taken_, None)

    assert init(taken_=None) == -1 and b"cvxpnpl_ransac_lo_init: bad arguments" in err() and b"d_lo_taken" in err()
    assert init(F=-1) == -1 and b"negative size" in err() and init(F=2**31) == -1 and b"int32" in err()

    def asm(F=2, A=2, act=p, off=p, tot=10, s2=p, s3=p, R=p, t=p, K=p, per=0, th=2.0, B=p, Q=p, cnt=p):
        return G.cvxpnpl_ransac_lo_assemble(F, A, act, off, tot, s2, s3, R, t, K, per, th, B, Q, cnt, None)

    named(asm, dict(act="d_active", off="d_offsets", s2="scene pointer", s3="scene pointer", R="d_R", t="d_t", K="d_K", B="d_B27", Q="d_Q45",
                    cnt="d_count"))
    assert b"cvxpnpl_ransac_lo_assemble: bad arguments" in err()
    assert asm(F=-1) == -1 and asm(A=-1) == -1 and asm(tot=-1) == -1 and b"negative size" in err()
    assert asm(F=2**31) == -1 and asm(A=2**31) == -1 and b"int32" in err()
    assert asm(per=2) == -1 and b"K_per_scene" in err()
    assert asm(th=nan) == -1 and b"thresh" in err() and asm(th=-1.0) == -1 and asm(th=float("inf")) == -1

    def upd(F=2, A=2, act=p, cap=8, conf=0.99, off=p, tot=10, fR=p, ft=p, fs=p, fc=p, K=p, per=0, s2=p, s3=p, th=2.0, oR=p, ot=p, head=p, best=p,
            mask=p, used=p, taken_=p, done=p):
        return G.cvxpnpl_ransac_lo_update(F, A, act, cap, conf, off, tot, fR, ft, fs, fc, K, per, s2, s3, th, oR, ot, head, best, mask, used, taken_,
                                          done, None)

    named(upd, dict(act="d_active", off="d_offsets", fR="d_fit_R", ft="d_fit_t", fs="d_fit_status", fc="d_fit_count", K="d_K", s2="scene pointer",
                    oR="d_io_R", ot="d_io_t", head="d_head", best="d_best", mask="d_mask", used="d_hyp_used", taken_="d_lo_taken", done="d_done"))
    assert b"cvxpnpl_ransac_lo_update: bad arguments" in err()
    for conf in (nan, 0.0, 1.0, -0.5, 1.5, float("inf")):
        assert upd(conf=conf) == -1 and b"confidence" in err(), conf
    assert upd(cap=-1) == -1 and b"cap" in err()
    assert upd(F=-2) == -1 and upd(A=-1) == -1 and upd(tot=-1) == -1 and upd(F=2**31) == -1 and upd(per=3) == -1 and upd(th=nan) == -1

    def host(F=2, A=2, act=p, off=p, tot=10, s2=p, s3=p, R=p, t=p, K=p, per=0, th=2.0, B=p, Q=p, cnt=p):
        return G.cvxpnpl_ransac_lo_assemble_host(F, A, act, off, tot, s2, s3, R, t, K, per, th, B, Q, cnt, 1)

    named(host, dict(act="active is null", off="offsets", s2="scene_2d", s3="scene_3d", R="R is null", t="t is null", K="K is null", B="B27", Q="Q45",
                     cnt="count"))
    assert b"cvxpnpl_ransac_lo_assemble_host: bad arguments" in err()
    assert host(F=-1) == -1 and host(A=-1) == -1 and host(tot=-1) == -1 and host(per=2) == -1 and host(th=nan) == -1

    # a zero-size call is a no-op whatever the pointers
    assert init(F=0, taken_=z) == 0
    for kw in (dict(F=0, tot=0), dict(A=0)):
        assert asm(act=z, off=z, s2=z, s3=z, R=z, t=z, K=z, B=z, Q=z, cnt=z, **kw) == 0
        assert host(act=z, off=z, s2=z, s3=z, R=z, t=z, K=z, B=z, Q=z, cnt=z, **kw) == 0
        assert upd(act=z, off=z, fR=z, ft=z, fs=z, fc=z, K=z, s2=z, s3=z, oR=z, ot=z, head=z, best=z, mask=z, used=z, taken_=z, done=z, **kw) == 0


def _compare(table, golden):
    problems = []
    for name, g in golden.items():
        r = table[name]
        for k in ("occupancy", "lds", "scratch", "sgpr_spill", "vgpr_spill"):
            if r[k] != g[k]:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]}")
        for k in ("vgpr", "agpr"):
            if r[k] > g[k] + REG_SLACK:
                problems.append(f"{name}: {k} {r[k]}, table says {g[k]} (+{REG_SLACK} allowed)")
        if g["scratch"] or g["vgpr_spill"] or g["sgpr_spill"]:
            problems.append(f"{name}: the table itself admits scratch or spills")
    return problems


def test_kernels_match_the_committed_resource_table(G):
    from cvxpnpl_amd import build as b

    assert os.path.exists(b.RANSAC_LO_RESOURCES) and os.path.getmtime(b.RANSAC_LO_RESOURCES) >= os.path.getmtime(b.RANSAC_LO_OUT) - 1
    table = b.kernel_resources(b.RANSAC_LO_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)
    g = golden["cvxnlo::lo_assemble_active_kernel"]
    assert g["lds"] == (4 * 60 + 60) * 8 + 4 * 8 + 4 * 4     # four wave sums and their total, four ballots, four counts
    assert g["vgpr"] + g["agpr"] <= 168 and g["occupancy"] == 3  # the loop's sums and the finish's B, Q are never live together
    assert golden["cvxnlo::lo_update_active_kernel"]["lds"] <= 128 and golden["cvxnlo::lo_init_kernel"]["lds"] == 0


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the other thirteen, none of theirs in this
    one's, and every one of the thirteen committed tables still holds."""
    from test_kernel_resources import _compare as compare_with_slack

    from cvxpnpl_amd import build as b

    b.build()
    others = {"": b.RESOURCES, "grad_": b.GRAD_RESOURCES, "ransac_": b.RANSAC_RESOURCES, "ransac_pnpl_": b.RANSAC_PNPL_RESOURCES,
              "refine_": b.REFINE_RESOURCES, "refine_grad_": b.REFINE_GRAD_RESOURCES, "refine_robust_": b.REFINE_ROBUST_RESOURCES,
              "refine_robust_grad_": b.REFINE_ROBUST_GRAD_RESOURCES, "ransac_adaptive_": b.RANSAC_ADAPTIVE_RESOURCES,
              "ransac_guided_": b.RANSAC_GUIDED_RESOURCES, "ransac_pnpl_adaptive_": b.RANSAC_PNPL_ADAPTIVE_RESOURCES,
              "refine_robust_auto_": b.REFINE_ROBUST_AUTO_RESOURCES, "ransac_msac_": b.RANSAC_MSAC_RESOURCES}
    assert len(others) == 13
    mine = b.kernel_resources(b.RANSAC_LO_RESOURCES)
    short = [k.split("::")[-1] for k in KERNELS]
    assert all(k.startswith("cvxnlo::") for k in mine)
    for lib, path in others.items():
        table = b.kernel_resources(path)
        assert table, lib
        assert not [k for k in table if "cvxnlo::" in k or any(n in k for n in short)], lib
        assert not set(table) & set(mine), lib
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", lib + "kernel_resources.json")))
        problems = compare_with_slack(table, golden, only=tuple(golden))   # occupancy and LDS exact, registers and scratch within the slack
        assert not problems, lib + "\n" + "\n".join(problems)


# ---- the assembly rule on the host: predicate, centre and sums

@pytest.fixture(scope="module", params=["shared_K", "per_scene_K"])
def case(request):
    return make_case(SIZES, per_scene_K=request.param == "per_scene_K")


def gathered_cost(case, f, mask):
    """(ok, B27, Q45) of scene f's masked correspondences by the host build of the device algorithm's assembly (tests/hostsim)"""
    import hostsim

    s = slice(case["off"][f], case["off"][f + 1])
    mk = mask[s]
    rc, B, Q = hostsim.assemble(case["x"][s][mk], case["X"][s][mk], None, None, scene_K(case, f))
    return rc == 0, B.reshape(27), pack45(Q)


@pytest.mark.parametrize("m_k", WIDEN)
@pytest.mark.parametrize("threads", [1, 3])
def test_host_assembly_equals_the_assembly_of_the_reference_set(G, case, m_k, threads):
    from cvxpnpl_amd.ransac import lo_assemble_host

    th = THRESH * m_k
    F = len(SIZES)
    assert case["margin"] > MARGIN
    active = np.arange(F)[::-1].copy()   # the compact layout: entry a is scene F - 1 - a
    Bt, Qt, cnt = lo_assemble_host(case["x"], case["X"], case["sizes"], case["K"], case["R"], case["t"], active, th, n_threads=threads)
    assert cnt.dtype == np.int32 and Bt.shape == (F, 27) and Qt.shape == (F, 45)
    mask = case["masks"][th]
    for a, f in enumerate(active):
        n_ref = int(mask[case["off"][f]:case["off"][f + 1]].sum())
        assert int(cnt[a]) == n_ref, (f, int(cnt[a]), n_ref)                 # exact
        ok, B_ref, Q_ref = gathered_cost(case, f, mask)
        if n_ref < 3 or not ok:
            assert np.isnan(Bt[a]).all() and np.isnan(Qt[a]).all(), f
        else:
            assert_cost_close(Bt[a], Qt[a], B_ref, Q_ref, (f, m_k))
    assert sum(int(c) >= 3 for c in cnt) >= F - 1                            # (the scene of four may take fewer than three)
    wide, narrow = case["masks"][THRESH * WIDEN[-1]], case["masks"][THRESH]
    assert (wide | narrow).sum() == wide.sum() > narrow.sum()                # the widened sets contain the narrow ones and differ


def test_host_assembly_active_list_behind_the_camera_and_too_few(G):
    """An active list shorter than F with an entry outside [0, F) (its rows stay as they were), a scene behind the camera and a scene of
    which two are taken (NaN, with the count reported); any thread count gives the same bits."""
    from cvxpnpl_amd.ransac import lo_assemble_host

    c = make_case((5, 65, 130, 300), seed=11, per_scene_K=True, thresholds=(THRESH,))
    R, t = c["R"].copy(), c["t"].copy()
    t[1] = -t[1]                                       # scene 1 behind the camera: nothing is taken
    x = c["x"].copy()
    s = slice(c["off"][2], c["off"][3])
    keep = np.flatnonzero(c["masks"][THRESH][s])[:2]   # scene 2: all but two of its correspondences moved far off
    moved = np.setdiff1d(np.arange(130), keep)
    x[s][moved] += 500.0
    c2 = dict(c, x=x)
    active = np.array([3, 7, 1, -1, 2], dtype=np.int32)
    out = [lo_assemble_host(x, c["X"], c["sizes"], c["K"], R, t, active, THRESH, n_threads=n) for n in (1, 2, 5)]
    for o in out[1:]:
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out[0], o))
    Bt, Qt, cnt = out[0]
    mask, _ = reference_masks(c2, R, t, THRESH)
    assert list(cnt) == [int(mask[c["off"][3]:].sum()), -1, 0, -1, 2]
    ok, B_ref, Q_ref = gathered_cost(c2, 3, mask)
    assert ok
    assert_cost_close(Bt[0], Qt[0], B_ref, Q_ref, "scene 3")
    assert np.isnan(Bt[1:]).all() and np.isnan(Qt[1:]).all()
    with pytest.raises(ValueError, match="R must be"):
        lo_assemble_host(x, c["X"], c["sizes"], c["K"], R[:2], t[:2], active, THRESH)


# ---- the reference itself, on hand-made numbers

def test_the_reference_schedule_rule_and_replay():
    assert [widen(k, 3, 2.0) for k in range(3)] == [2.0, 1.5, 1.0] and widen(0, 1, 2.0) == 1.0 and [widen(k, 2, 1.5) for k in range(2)] == [1.5, 1.0]
    assert take_fit(0, 4, 7, 7) and take_fit(2, 9, 8, 7) and not take_fit(0, 4, 6, 7) and not take_fit(3, 9, 9, 7) and not take_fit(1, 9, 9, 7)
    assert not take_fit(0, 3, 9, 7)
    counts = np.zeros((3, 24), dtype=np.int64)
    status = np.zeros((3, 24), dtype=np.int64)
    counts[0, 3] = 7          # scene 0: 7 of 10 after round 0 (N = 25 > 8: goes on) -- the refit finds all 10 and stops it there
    counts[1, 2] = 7          # scene 1: the same without a usable refit: runs to the cap
    counts[2, 1] = 6          # scene 2: a refit of an equal count is taken (tie), one short is not; round 1 brings 7, strictly more
    counts[2, 12] = 7
    lo_counts = np.zeros((3, 3, 2), dtype=np.int64)
    lo_usable = np.ones((3, 3, 2), dtype=bool)
    lo_counts[0, 0] = (8, 10)
    lo_counts[1], lo_usable[1] = 10, False
    lo_counts[2, 0] = (6, 5)
    lo_counts[2, 1] = (6, 7)
    lo_counts[2, 2] = (3, 3)
    out = simulate_lo(counts, status, [10, 10, 10], lo_counts, lo_usable, 0.99, 8, 24)
    assert list(out["hyp_used"]) == [8, 24, 24] and list(out["best"]) == [10, 7, 7] and list(out["lo_taken"]) == [2, 0, 2]
    assert list(out["winner"]) == [3, 2, 12] and list(out["from_fit"]) == [True, False, True]
    assert [list(a) for a in out["active"]] == [[0, 1, 2], [1, 2], [1, 2]] and [list(d) for d in out["done"]] == [[True, False, False], [False, False], [True, True]]
    plain = simulate_lo(counts, status, [10, 10, 10], np.zeros((3, 3, 0)), np.zeros((3, 3, 0), dtype=bool), 0.99, 8, 24)
    from ransac_adaptive_reference import simulate

    ref = simulate(counts, status, [10, 10, 10], 0.99, 8, 24)
    assert all(np.array_equal(plain[k], ref[k]) for k in ("hyp_used", "winner", "best", "certified")) and (out["hyp_used"] <= plain["hyp_used"]).all()


# ---- the keywords

def _scene(m, rs):
    return rs.random_sample((m, 2)), rs.random_sample((m, 3))


def test_lo_keywords_are_validated_on_the_host_after_the_earlier_checks():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import cvxpnpl_amd
    from cvxpnpl_amd.ransac import lo_thresholds, ransac_pnp_batch

    par = inspect.signature(ransac_pnp_batch).parameters
    assert par["local_opt"].default == 0 and par["lo_widen"].default == 1.0
    for name in ("lo_init", "lo_assemble_active", "lo_update_active", "lo_assemble_host", "lo_thresholds"):
        assert callable(getattr(cvxpnpl_amd, name)), name
    assert lo_thresholds(2.0, 3, 2.0) == [2.0 * widen(k, 3, 2.0) for k in range(3)] == [4.0, 3.0, 2.0]
    assert lo_thresholds(3.0, 1, 2.0) == [3.0] and lo_thresholds(2.0, 0, 2.0) == [] and lo_thresholds(2.0, 2, 1.0) == [2.0, 2.0]
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3 = _scene(10, rs)
    b2, b3 = _scene(7, rs)
    call = lambda **kw: ransac_pnp_batch([a2, b2], [a3, b3], K, **kw)  # noqa: E731
    for bad in (-1, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="local_opt"):
            call(confidence=0.99, local_opt=bad)
    for bad in (0.5, float("nan"), float("inf"), -2.0, "wide", None):
        with pytest.raises(ValueError, match="lo_widen"):
            call(confidence=0.99, local_opt=1, lo_widen=bad)
    with pytest.raises(ValueError, match="lo_widen"):
        call(lo_widen=0.0)                                    # (checked with local_opt = 0 too)
    with pytest.raises(ValueError, match="local_opt needs confidence"):
        call(local_opt=1)
    with pytest.raises(ValueError, match="local_opt with scoring='msac'"):
        call(confidence=0.99, local_opt=2, scoring="msac")
    # the earlier errors still come first, in their order
    with pytest.raises(ValueError, match="needs 4"):
        ransac_pnp_batch([a2, b2[:3]], [a3, b3[:3]], K, local_opt=-1)
    with pytest.raises(ValueError, match="confidence"):
        call(confidence=2.0, n_hyp=0, scoring="bad", local_opt=-1)
    with pytest.raises(ValueError, match="seeds"):
        call(seed=[1, 2, 3], n_hyp=0, scoring="bad", local_opt=-1)
    with pytest.raises(ValueError, match="n_hyp"):
        call(n_hyp=0, pool_full=3, scoring="bad", local_opt=-1)
    with pytest.raises(ValueError, match="pool_full"):
        call(pool_full=3, scoring="bad", local_opt=-1)
    with pytest.raises(ValueError, match="scoring"):
        call(scoring="bad", local_opt=-1)


# ---- the experiment that motivates the library, on the host build of the device algorithm (tests/hostsim) and the reference only

def test_local_optimisation_stops_scenes_earlier():
    """24 scenes of 100 correspondences (50 % clutter, 1 px noise), thresh 2, confidence 0.99, rounds of 64 under a cap of 1024, the
    draws the device sampler's; local_opt=3, lo_widen=2 at the round solves' eps=1e-6 / max_iters=100.  No scene draws more with LO
    than without (exact: the theorem of DESIGN.md section 24), and the hypotheses drawn, summed over the scenes, fall from 6144 to 3776:
    measured ratio 0.61 (one step per round: 4480, 0.73; mean inliers of the running best 40.1 -> 44.6).  The bound 0.81 is half-way
    between the measured ratio and no effect."""
    from cvxpnpl_amd import synth

    plain, lo = [], []
    for f in range(24):
        d = synth.make_ransac(1, n_corr=100, outlier_frac=0.5, sigma=1.0, seed=100 + f)
        s = SceneReplay(d, f, 1024, THRESH)
        plain.append(s.run(0.99, 64))
        lo.append(s.run(0.99, 64, local_opt=3, lo_widen=2.0))
    used_p, used_l = np.array([r["hyp_used"] for r in plain]), np.array([r["hyp_used"] for r in lo])
    ratio = used_l.sum() / used_p.sum()
    print(f"hypotheses drawn: plain {used_p.sum()}, LO {used_l.sum()}, ratio {ratio:.3f};  mean inliers {np.mean([r['best'] for r in plain]):.1f} -> "
          f"{np.mean([r['best'] for r in lo]):.1f};  refits taken {sum(r['lo_taken'] for r in lo)}")
    assert (used_l <= used_p).all(), (used_l, used_p)
    assert all(r["lo_taken"] == 0 for r in plain) and sum(r["lo_taken"] for r in lo) > 0
    assert ratio <= 0.81, ratio
