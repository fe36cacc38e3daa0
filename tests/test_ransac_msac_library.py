"""The library of MSAC scoring (libcvxpnpl_amd_ransac_msac.so, include/cvxpnpl_amd_ransac_msac.h): it builds by
cross-compilation, exports what its header declares and nothing else, rejects bad arguments before it touches a device, keeps its kernels
free of scratch and spills (tests/golden/ransac_msac_kernel_resources.json), leaves the other twelve libraries alone and lists its
dependencies exactly; its arithmetic on the host against the numpy reference (tests/ransac_msac_reference.py); the host-side validation
of ransac_pnp_batch(scoring=...); and the experiment that motivates it, on the host build of the device algorithm.  No GPU needed."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_msac_reference import (argmax_first, gain_count, gain_count_scenes, perturbed_poses, rotation_error_deg, simulate_msac)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_msac_kernel_resources.json")
REG_SLACK = 8  # VGPRs / AGPRs an edit may move (tests/test_kernel_resources.py); occupancy, LDS, scratch and spills are exact
KERNELS = ("cvxnm::score_scenes_msac_kernel", "cvxnm::score_active_msac_kernel", "cvxnm::select_scenes_msac_kernel", "cvxnm::msac_init_kernel",
           "cvxnm::round_update_msac_kernel")
GAIN_TOL = 1e-9      # absolute, on gains of up to M = 700: the float64 reference is within 6e-13 of its long-double twin at M = 100
TWIN_TOL = 1e-10     # the reference against its long-double twin on the inputs used here: what keeps GAIN_TOL's margin honest
MARGIN = 1e-9        # every |r^2 - tau^2| / tau^2 of the inputs is above this, so that an exactly equal count is a fair demand
THRESH = 4.0


def make_case(sizes, H, seed=7, thresh=THRESH, per_scene_K=False, outliers=None):
    """Scenes of synth.make_ransac (30 % clutter unless `outliers` gives a share per scene, 1 px noise) of the given sizes and H host-made poses per scene around the ground truth
    (rotations of 0 .. 2 degrees, translations of 0 .. 5 %: gains from M down to 0).  The seed is redrawn until no residual sits within
    MARGIN of the threshold.  Returns a dict of numpy arrays: x [sum M,2], X [sum M,3], sizes, K, R [F*H,3,3], t [F*H,3], and the
    reference's gain, count."""
    from cvxpnpl_amd import synth

    for attempt in range(8):
        rs = np.random.RandomState(seed + 1000 * attempt)
        xs, Xs, Rs, ts, Ks = [], [], [], [], []
        for f, m in enumerate(sizes):
            K = np.array(synth.K_KINECT, dtype=np.float64)
            if per_scene_K:
                K[0, 0] *= 1.0 + 0.02 * f
                K[1, 1] *= 1.0 - 0.02 * f
            d = synth.make_ransac(1, n_corr=m, outlier_frac=0.3 if outliers is None else outliers[f], sigma=1.0, seed=seed + 1000 * attempt + f, K=K)
            R, t = perturbed_poses(d["R_gt"], d["t_gt"], H, rs)
            xs.append(d["scene_2d"]); Xs.append(d["scene_3d"]); Rs.append(R); ts.append(t); Ks.append(K)
        case = {"x": np.concatenate(xs), "X": np.concatenate(Xs), "sizes": list(sizes), "K": np.stack(Ks) if per_scene_K else Ks[0],
                "R": np.concatenate(Rs), "t": np.concatenate(ts), "thresh": thresh, "H": H}
        case["gain"], case["count"], margin = gain_count_scenes(case["x"], case["X"], sizes, case["K"], case["R"], case["t"], thresh)
        if margin > MARGIN:
            case["margin"] = margin
            return case
    raise AssertionError("no seed keeps every residual away from the threshold")


@pytest.fixture(scope="module")
def G():
    from cvxpnpl_amd import _lib, build

    build.build_ransac_msac()
    assert os.path.exists(build.RANSAC_MSAC_OUT)
    return _lib.ransac_msac_lib()


def test_header_symbols_are_exported_and_nothing_else(G):
    from cvxpnpl_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvxpnpl_amd_ransac_msac.h")).read(), flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(cvxpnpl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.RANSAC_MSAC_EXPORTS), declared ^ set(_lib.RANSAC_MSAC_EXPORTS)
    assert all(name.startswith("cvxpnpl_ransac_msac_") for name in declared)
    for name in declared:
        assert getattr(G, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", build.RANSAC_MSAC_OUT], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cvxpnpl_")}
    assert defined == declared, defined ^ declared


def test_same_compile_flags_as_the_ransac_library_and_exact_dependencies():
    """The thirteenth pair is named apart from the twelve tests/test_build_deps.py pins; the property it checks is checked here."""
    from test_build_deps import include_closure

    from cvxpnpl_amd import build as b

    assert b.ransac_msac_command("x")[:-1] == b.ransac_compile_cmd("x")[:-1]
    sources = [c for c in b.ransac_msac_command("x") if c.endswith((".hip", ".cpp"))]
    assert sources == [b.RANSAC_MSAC_SRC]
    listed = [os.path.realpath(d) for d in b.RANSAC_MSAC_SOURCES]
    assert len(listed) == len(set(listed))
    closure = include_closure(sources)
    assert set(listed) == closure, (sorted(closure - set(listed)), sorted(set(listed) - closure))


def test_bad_arguments_are_rejected_without_gpu(G):
    p = C.c_void_p(8)  # a non-null pointer that is never followed: every call below returns before it launches anything
    err = G.cvxpnpl_ransac_msac_last_error
    nan, z = float("nan"), None

    def named(call, names, **fixed):
        for name, word in names.items():
            assert call(**{name: None}, **fixed) == -1, name
            assert word.encode() in err(), (name, err())

    def score(F=2, H=8, off=p, tot=10, R=p, t=p, st=None, um=5, K=p, per=0, s2=p, s3=p, th=2.0, gain=p, cnt=p):
        return G.cvxpnpl_ransac_msac_score_scenes(F, H, off, tot, R, t, st, um, K, per, s2, s3, th, gain, cnt, None)

    named(score, dict(off="d_offsets", R="d_R", t="d_t", K="d_K", gain="d_gain", cnt="d_count", s2="scene pointer", s3="scene pointer"))
    assert b"cvxpnpl_ransac_msac_score_scenes: bad arguments" in err()
    assert score(F=-1) == -1 and b"negative size" in err()
    assert score(tot=-1) == -1 and score(H=-1) == -1 and b"n_hyp" in err()
    assert score(per=2) == -1 and b"K_per_scene" in err()
    assert score(th=nan) == -1 and b"thresh" in err() and score(th=-1.0) == -1 and score(th=float("inf")) == -1

    def active(F=2, A=2, act=p, Hr=8, off=p, tot=10, R=p, t=p, st=None, um=5, K=p, per=0, s2=p, s3=p, th=2.0, gain=p, cnt=p):
        return G.cvxpnpl_ransac_msac_score_active(F, A, act, Hr, off, tot, R, t, st, um, K, per, s2, s3, th, gain, cnt, None)

    named(active, dict(act="d_active", off="d_offsets", R="d_R", t="d_t", K="d_K", gain="d_gain", cnt="d_count", s3="scene pointer"))
    assert b"cvxpnpl_ransac_msac_score_active: bad arguments" in err()
    assert active(F=-1) == -1 and active(A=-1) == -1 and active(tot=-1) == -1 and active(Hr=-1) == -1 and b"n_round" in err()
    assert active(F=2**31) == -1 and active(per=2) == -1 and active(th=nan) == -1

    def select(F=2, H=8, off=p, tot=10, gain=p, R=p, t=p, st=p, K=p, per=0, s2=p, s3=p, th=2.0, oR=p, ot=p, head=p, mask=p, score=p):
        return G.cvxpnpl_ransac_msac_select_scenes(F, H, off, tot, gain, R, t, st, K, per, s2, s3, th, oR, ot, head, mask, score, None)

    named(select, dict(off="d_offsets", gain="d_gain", R="d_R", t="d_t", st="d_status", K="d_K", oR="d_out_R", ot="d_out_t", head="d_head",
                       mask="d_mask", score="d_score", s2="scene pointer"))
    assert b"cvxpnpl_ransac_msac_select_scenes: bad arguments" in err()
    assert select(H=0) == -1 and b"at least one hypothesis" in err()
    assert select(F=-1) == -1 and select(tot=-1) == -1 and select(F=2**31) == -1 and select(per=3) == -1 and select(th=nan) == -1

    def init(F=2, bg=p):
        return G.cvxpnpl_ransac_msac_init(F, bg, None)

    assert init(bg=None) == -1 and b"cvxpnpl_ransac_msac_init: bad arguments" in err() and b"d_best_gain" in err()
    assert init(F=-1) == -1 and init(F=2**31) == -1

    def update(F=2, A=2, act=p, h0=0, Hr=8, cap=8, conf=0.99, off=p, tot=10, gain=p, cnt=p, R=p, t=p, st=p, K=p, per=0, s2=p, s3=p, th=2.0, oR=p,
               ot=p, head=p, best=p, bg=p, mask=p, used=p, done=p):
        return G.cvxpnpl_ransac_msac_update(F, A, act, h0, Hr, cap, conf, off, tot, gain, cnt, R, t, st, K, per, s2, s3, th, oR, ot, head, best, bg,
                                            mask, used, done, None)

    named(update, dict(act="d_active", off="d_offsets", gain="d_gain", cnt="d_count", R="d_R", t="d_t", st="d_status", K="d_K", oR="d_out_R",
                       ot="d_out_t", head="d_head", best="d_best", bg="d_best_gain", mask="d_mask", used="d_hyp_used", done="d_done"))
    assert b"cvxpnpl_ransac_msac_update: bad arguments" in err()
    for conf in (nan, 0.0, 1.0, -0.5, 1.5, float("inf")):
        assert update(conf=conf) == -1 and b"confidence" in err(), conf
    assert update(Hr=-8) == -1 and update(h0=-1) == -1 and update(cap=-1, Hr=0) == -1
    assert update(h0=4, Hr=8, cap=11) == -1 and b"exceeds cap" in err()
    assert update(Hr=0) == -1 and b"at least one hypothesis" in err()
    assert update(F=-2) == -1 and update(A=-1) == -1 and update(per=3) == -1 and update(th=nan) == -1

    def host(F=2, H=8, off=p, tot=10, R=p, t=p, st=None, um=5, K=p, per=0, s2=p, s3=p, th=2.0, gain=p, cnt=p):
        return G.cvxpnpl_ransac_msac_score_host(F, H, off, tot, R, t, st, um, K, per, s2, s3, th, gain, cnt, 1)

    named(host, dict(off="offsets", R="R is null", t="t is null", K="K is null", gain="gain", cnt="count", s2="scene_2d", s3="scene_3d"))
    assert b"cvxpnpl_ransac_msac_score_host: bad arguments" in err()
    assert host(F=-1) == -1 and host(H=-1) == -1 and host(tot=-1) == -1 and host(per=2) == -1 and host(th=nan) == -1

    # a zero-size call is a no-op whatever the pointers
    assert score(F=0, tot=0, off=z, R=z, t=z, K=z, s2=z, s3=z, gain=z, cnt=z) == 0
    assert host(F=0, tot=0, off=z, R=z, t=z, K=z, s2=z, s3=z, gain=z, cnt=z) == 0
    assert score(H=0, R=z, t=z, K=z, gain=z, cnt=z) == 0 and host(H=0, off=z, R=z, t=z, K=z, s2=z, s3=z, gain=z, cnt=z) == 0
    for kw in (dict(F=0, tot=0), dict(A=0)):
        assert active(act=z, off=z, R=z, t=z, K=z, s2=z, s3=z, gain=z, cnt=z, **kw) == 0
        assert update(act=z, off=z, gain=z, cnt=z, R=z, t=z, st=z, K=z, s2=z, s3=z, oR=z, ot=z, head=z, best=z, bg=z, mask=z, used=z, done=z, **kw) == 0
    assert active(Hr=0, R=z, t=z, K=z, gain=z, cnt=z) == 0
    assert select(F=0, tot=0, off=z, gain=z, R=z, t=z, st=z, K=z, s2=z, s3=z, oR=z, ot=z, head=z, mask=z, score=z) == 0
    assert init(F=0, bg=z) == 0


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

    assert os.path.exists(b.RANSAC_MSAC_RESOURCES) and os.path.getmtime(b.RANSAC_MSAC_RESOURCES) >= os.path.getmtime(b.RANSAC_MSAC_OUT) - 1
    table = b.kernel_resources(b.RANSAC_MSAC_RESOURCES)
    golden = json.load(open(GOLDEN))
    assert set(table) == set(golden) == set(KERNELS), set(table) ^ set(golden)
    problems = _compare(table, golden)
    assert not problems, "\n".join(problems)
    for k, g in golden.items():
        if "::score_" in k:
            assert g["lds"] == 512 * 5 * 8, k        # LDS is the scoring tile's ...
        else:
            assert g["lds"] <= 128, k                # ... and a few words for the cross-wave reductions of the selection and the update


def test_the_other_libraries_are_left_alone():
    """The new kernels live in their own library: none of them appears in the remarks of the other twelve, none of theirs in this one's,
    and the tables of the libraries whose headers this one includes (ransac, ransac_adaptive) still hold."""
    from cvxpnpl_amd import build as b

    b.build()
    others = {"solver": b.RESOURCES, "grad": b.GRAD_RESOURCES, "ransac": b.RANSAC_RESOURCES, "ransac_pnpl": b.RANSAC_PNPL_RESOURCES,
              "refine": b.REFINE_RESOURCES, "refine_grad": b.REFINE_GRAD_RESOURCES, "refine_robust": b.REFINE_ROBUST_RESOURCES,
              "refine_robust_grad": b.REFINE_ROBUST_GRAD_RESOURCES, "ransac_adaptive": b.RANSAC_ADAPTIVE_RESOURCES,
              "ransac_guided": b.RANSAC_GUIDED_RESOURCES, "ransac_pnpl_adaptive": b.RANSAC_PNPL_ADAPTIVE_RESOURCES,
              "refine_robust_auto": b.REFINE_ROBUST_AUTO_RESOURCES}
    tables = {lib: b.kernel_resources(path) for lib, path in others.items()}
    mine = b.kernel_resources(b.RANSAC_MSAC_RESOURCES)
    short = [k.split("::")[-1] for k in KERNELS]
    for lib, table in tables.items():
        assert table, lib
        assert not [k for k in table if "cvxnm::" in k or any(n in k for n in short)], lib
        assert not set(table) & set(mine), lib
    assert all(k.startswith("cvxnm::") for k in mine)
    for lib, name in (("ransac", "ransac_kernel_resources.json"), ("ransac_adaptive", "ransac_adaptive_kernel_resources.json")):
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert set(tables[lib]) == set(golden), (lib, set(tables[lib]) ^ set(golden))
        problems = _compare(tables[lib], golden)
        assert not problems, "\n".join(problems)


SIZES = (4, 63, 64, 65, 511, 512, 513, 700)


@pytest.fixture(scope="module")
def case():
    return make_case(SIZES, 24)


def test_inputs_stay_away_from_the_threshold_and_the_reference_agrees_with_its_long_double_twin(case):
    assert case["margin"] > MARGIN, case["margin"]
    g64, c64 = case["gain"], case["count"]
    gld, cld, _ = gain_count_scenes(case["x"], case["X"], case["sizes"], case["K"], case["R"], case["t"], case["thresh"], dtype=np.longdouble)
    worst = float(np.max(np.abs(g64.astype(np.longdouble) - gld)))
    print(f"reference float64 against long double: worst |gain difference| {worst:.2e}, least margin to the threshold {case['margin']:.2e}")
    assert np.array_equal(c64, cld)
    assert worst <= TWIN_TOL, worst
    F, H = len(SIZES), case["H"]
    g = g64.reshape(F, H)
    assert (g[:, 0] > 0.3 * np.array(SIZES)).all() and (g.min(axis=1) < 0.2 * np.array(SIZES)).all()   # the gains span the range
    assert ((g64 >= 0) & (g64 <= c64)).all()


@pytest.mark.parametrize("threads", [1, 3])
def test_msac_gain_host_equals_the_reference(G, case, threads):
    from cvxpnpl_amd.ransac import msac_gain_host

    gain, count = msac_gain_host(case["x"], case["X"], case["sizes"], case["K"], case["R"], case["t"], case["thresh"], n_threads=threads)
    worst = float(np.max(np.abs(gain - case["gain"])))
    print(f"msac_gain_host against the reference: worst |gain difference| {worst:.2e} over gains up to {case['gain'].max():.1f}")
    assert count.dtype == np.int32 and np.array_equal(count, case["count"])
    assert worst <= GAIN_TOL, worst


def test_msac_gain_host_status_rule_nan_poses_and_per_scene_K(G):
    from cvxpnpl_amd.ransac import msac_gain_host

    c = make_case((5, 65, 130), 6, seed=11, per_scene_K=True)
    n = len(c["R"])
    status = np.array([0, 1, 2, 3, 0, 2] * 3, dtype=np.int32)
    R, t = c["R"].copy(), c["t"].copy()
    R[4] = np.nan                  # a usable status on a NaN pose: every comparison is false
    t[11] = -t[11]                 # scene 1, pose 5: the scene behind the camera
    ref_g, ref_c, _ = gain_count_scenes(c["x"], c["X"], c["sizes"], c["K"], R, t, c["thresh"], status=status)
    gain, count = msac_gain_host(c["x"], c["X"], c["sizes"], c["K"], R, t, c["thresh"], status=status)
    assert np.array_equal(count, ref_c) and np.max(np.abs(gain - ref_g)) <= GAIN_TOL
    assert (gain[np.isin(status, (1, 3))] == 0.0).all() and (count[np.isin(status, (1, 3))] == 0).all()
    assert gain[4] == 0.0 and count[4] == 0 and gain[11] == 0.0 and count[11] == 0
    assert gain[0] > 0 and n == 18
    g0, c0 = msac_gain_host(c["x"], c["X"], c["sizes"], c["K"], R, t, 0.0, status=status)   # thresh = 0: nothing passes, no 0 / 0
    assert (g0 == 0.0).all() and (c0 == 0).all()


def test_the_reference_selection_and_replay():
    """argmax_first and simulate_msac on hand-made numbers: NaN and negative gains never win, the first of equal maxima does, a later round
    takes over only by a strictly greater gain, and the stopping rule reads the count of the running MSAC winner."""
    nan = float("nan")
    assert argmax_first([nan, -1.0, 0.0]) == 0 and argmax_first([nan, -3.0, 2.0, 2.0]) == 2 and argmax_first([0.0, 0.0]) == 0
    gains = np.zeros((3, 20))
    counts = np.zeros((3, 20), dtype=np.int64)
    status = np.zeros((3, 20), dtype=np.int64)
    gains[0, 3], counts[0, 3] = 9.5, 10                       # all inliers in round 0: N = 0
    gains[1, 2] = gains[1, 9] = 6.0                           # an exact tie across rounds: index 2 stays ...
    counts[1, 2], counts[1, 9] = 7, 8                         # ... although the later one counts more
    gains[2, 1], counts[2, 1] = 4.0, 7                        # round 0: count 7 of 10 (N = 25: the scene goes on) ...
    gains[2, 12], counts[2, 12] = 5.5, 6                      # ... round 1: a higher gain with a LOWER count takes over
    out = simulate_msac(gains, counts, status, [10, 10, 10], 0.99, 8, 20)
    assert list(out["winner"]) == [3, 2, 12] and list(out["best"]) == [10, 7, 6] and list(out["best_gain"]) == [9.5, 6.0, 5.5]
    assert list(out["hyp_used"]) == [8, 20, 20] and [list(a) for a in out["active"]] == [[0, 1, 2], [1, 2], [1, 2]]


def _scene(m, rs):
    return rs.random_sample((m, 2)), rs.random_sample((m, 3))


def test_scoring_keyword_is_validated_on_the_host_after_the_earlier_checks():
    """Every ValueError below is raised before a GPU is asked for: this test runs on a machine without one."""
    import cvxpnpl_amd
    from cvxpnpl_amd.ransac import ransac_pnp_batch

    assert inspect.signature(ransac_pnp_batch).parameters["scoring"].default == "count"
    for name in ("score_scenes_msac", "score_active_msac", "select_scenes_msac", "update_active_msac", "adaptive_init_msac", "msac_gain_host"):
        assert callable(getattr(cvxpnpl_amd, name)), name
    rs = np.random.RandomState(0)
    K = np.eye(3)
    a2, a3 = _scene(10, rs)
    b2, b3 = _scene(7, rs)
    for bad in ("MSAC", "ransac", "", None, 1):
        with pytest.raises(ValueError, match="scoring"):
            ransac_pnp_batch([a2, b2], [a3, b3], K, scoring=bad)
    # the earlier errors still come first, in their order
    with pytest.raises(ValueError, match="needs 4"):
        ransac_pnp_batch([a2, b2[:3]], [a3, b3[:3]], K, scoring="bad")
    with pytest.raises(ValueError, match="confidence"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, confidence=2.0, n_hyp=0, scoring="bad")
    with pytest.raises(ValueError, match="seeds"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, seed=[1, 2, 3], n_hyp=0, scoring="bad")
    with pytest.raises(ValueError, match="n_hyp"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, n_hyp=0, pool_full=3, scoring="bad")
    with pytest.raises(ValueError, match="pool_full"):
        ransac_pnp_batch([a2, b2], [a3, b3], K, pool_full=3, scoring="bad")


# ---- the experiment that motivates the library, on the host build of the device algorithm (tests/hostsim) and the reference only

def winners_by_count_and_msac(scene, idx, sol, thresh):
    """One scene's winners among the solved minimal sets idx: (hypothesis by count, hypothesis by gain), both the first of equal maxima;
    a hypothesis whose solve status is neither 0 nor 2 scores nothing."""
    gain, count, _ = gain_count(scene["scene_2d"], scene["scene_3d"], scene["K"], sol["R"], sol["t"], thresh)
    ok = np.isin(sol["status"], (0, 2))
    return int(np.argmax(np.where(ok, count, 0))), argmax_first(np.where(ok, gain, 0.0))


def test_msac_winner_is_closer_to_the_truth_than_the_count_winner():
    """48 scenes of 100 correspondences (30 % clutter, 1 px noise), 128 hypotheses each drawn as the device sampler draws them, thresh = 4:
    most scenes tie on the count and the lowest index decides; the MSAC winner's mean rotation error is at most 0.85 of the count
    winner's (measured: 0.68; 0.85 is half-way to no effect)."""
    import hostsim
    from cvxpnpl_amd import synth

    n_scenes, n_hyp, thresh = 48, 128, 4.0
    err_c, err_m, ties = [], [], 0
    for f in range(n_scenes):
        d = synth.make_ransac(1, n_corr=100, outlier_frac=0.3, sigma=1.0, seed=100 + f)
        idx = synth.philox_minimal_sets(n_hyp, 100, 4, f)
        sol = hostsim.solve_batch(d["scene_2d"][idx], d["scene_3d"][idx], None, None, d["K"], hostsim.default_opts(eps=1e-6, max_iters=100))
        hc, hm = winners_by_count_and_msac(d, idx, sol, thresh)
        _, count, _ = gain_count(d["scene_2d"], d["scene_3d"], d["K"], sol["R"], sol["t"], thresh)
        count = np.where(np.isin(sol["status"], (0, 2)), count, 0)
        ties += int((count == count.max()).sum() > 1)
        err_c.append(rotation_error_deg(sol["R"][hc], d["R_gt"]))
        err_m.append(rotation_error_deg(sol["R"][hm], d["R_gt"]))
    err_c, err_m = np.array(err_c), np.array(err_m)
    print(f"count winner: mean {err_c.mean():.3f} deg, median {np.median(err_c):.3f} deg;  MSAC winner: mean {err_m.mean():.3f} deg, median "
          f"{np.median(err_m):.3f} deg;  ratio {err_m.mean() / err_c.mean():.2f};  {ties} of {n_scenes} scenes tie on the count;  MSAC better "
          f"{int((err_m < err_c).sum())}, equal {int((err_m == err_c).sum())}, worse {int((err_m > err_c).sum())}")
    assert err_m.mean() <= 0.85 * err_c.mean(), (err_m.mean(), err_c.mean())
