"""ctypes binding of the C ABI (include/cvxpnpl_amd.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``python -m cvxpnpl_amd.build``.  There is NO CPU fallback: if the library is missing,
or no GPU is visible, the solver entry points raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CVXPNPL_AMD_LIB: diagnostics only (tools/phase_profile.py loads an instrumented build through it)
LIB_PATH = os.environ.get("CVXPNPL_AMD_LIB") or os.path.join(_HERE, "libcvxpnpl_amd.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

# every symbol include/cvxpnpl_amd.h declares
EXPORTS = (
    "cvxpnpl_default_opts", "cvxpnpl_opts_size", "cvxpnpl_solve_batch", "cvxpnpl_solve_cost_batch", "cvxpnpl_recover_multi", "cvxpnpl_recover_multi_batch", "cvxpnpl_recover_multi_device", "cvxpnpl_assemble_batch",
    "cvxpnpl_assemble_large_batch", "cvxpnpl_assemble_large_scratch_bytes",
    "cvxpnpl_score_hypotheses", "cvxpnpl_select_best", "cvxpnpl_refit_update", "cvxpnpl_sample_minimal_sets", "cvxpnpl_assemble_subsets", "cvxpnpl_pack_results", "cvxpnpl_stream_write_value", "cvxpnpl_stream_wait_value", "cvxpnpl_stream_wait_value_bounded", "cvxpnpl_stream_wait_gave_up", "cvxpnpl_synth_batch", "cvxpnpl_pose_errors", "cvxpnpl_disambiguate",
    "cvxpnpl_workspace_bytes", "cvxpnpl_set_workspace", "cvxpnpl_release_workspace", "cvxpnpl_calibration_copy", "cvxpnpl_ipm_batch",
    "cvxpnpl_event_create", "cvxpnpl_event_record", "cvxpnpl_event_elapsed_ms", "cvxpnpl_event_destroy",
    "cvxpnpl_last_error", "cvxpnpl_last_layout", "cvxpnpl_version", "cvxpnpl_device_count",
)

VARIANT_FULL, VARIANT_RC = 0, 1
STATUS_NAMES = {0: "certified", 1: "rank>1", 2: "uncertified", 3: "nonfinite", 4: "reflection"}


class Opts(C.Structure):
    """cvxpnpl_opts_t"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("eps", C.c_double), ("max_iters", C.c_int32), ("rho", C.c_double), ("alpha", C.c_double),
        ("first_check", C.c_int32), ("check_every", C.c_int32), ("res_tol", C.c_double),
        ("jacobi_sweeps", C.c_int32), ("jacobi_tol", C.c_double), ("warm_start", C.c_int32), ("rho_tail", C.c_double), ("tail_from", C.c_int32), ("lane_iters", C.c_int32), ("layout", C.c_int32),
        ("variant", C.c_int32), ("adapt_every", C.c_int32), ("adapt_from", C.c_int32), ("adapt_mu", C.c_double), ("adapt_tau", C.c_double),
        ("stall_from", C.c_int32), ("stall_lam", C.c_double), ("stall_res", C.c_double), ("stall_drop", C.c_double), ("rescue_from", C.c_int32),
        ("f32_sweeps_until", C.c_int32), ("sweep_schedule", C.c_int32), ("dual_shift", C.c_double), ("dual_refine", C.c_int32),
    ]


class LibraryMissing(RuntimeError):
    pass


_loaded = {}


def _load(path, exports, set_argtypes, missing=None, optional=()):
    """Load a library of `exports` once (loudly).  Every export returns int but *_last_error and *_version, which return a string;
    set_argtypes(L) gives the argument types, and the return type of an export that returns something else.  missing: the message of a
    library that is not there; optional: exports the library may lack."""
    L = _loaded.get(path)
    if L is None:
        if not os.path.exists(path):
            raise LibraryMissing(missing or f"{path} is missing: the HIP extension has not been built (`python -m cvxpnpl_amd.build`)")
        L = C.CDLL(path)
        for name in exports:
            if name not in optional or hasattr(L, name):
                getattr(L, name).restype = C.c_char_p if name.endswith(("_last_error", "_version")) else C.c_int
        set_argtypes(L)
        _loaded[path] = L
    return L


# an A/B library of an earlier round, loaded through the diagnostics variable, may predate these entries; the product library must have them
_SOLVER_OPTIONAL = ("cvxpnpl_stream_wait_value_bounded", "cvxpnpl_stream_wait_gave_up", "cvxpnpl_select_best", "cvxpnpl_refit_update",
                    "cvxpnpl_last_layout")


def _solver_argtypes(L):
    p, i32, i64, u64, f64, size = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_size_t
    corr = [i64, i32, p, p, i32, p, p, p, i32]  # batch, n_p, pts_2d, pts_3d, n_l, line_2d, line_3d, K, K_per_problem
    outs = [p, p, p, p, p, p, p]                # R, t, status, iters, cost, Z, work
    argtypes = {
        "cvxpnpl_default_opts": [C.POINTER(Opts)], "cvxpnpl_opts_size": [],
        "cvxpnpl_solve_batch": corr + [C.POINTER(Opts)] + outs + [p],
        "cvxpnpl_solve_cost_batch": [i64, p, p, C.POINTER(Opts)] + outs + [p],
        "cvxpnpl_assemble_batch": corr + [p, p, p],
        "cvxpnpl_assemble_large_scratch_bytes": [i64, i32, i32],
        "cvxpnpl_assemble_large_batch": corr + [p, p, p, size, p],
        "cvxpnpl_recover_multi": [_dp, _dp, _dp, _dp, _dp],
        "cvxpnpl_recover_multi_batch": [i64, _ip, _dp, _dp, _dp, _dp, _dp, _ip, i32],
        "cvxpnpl_recover_multi_device": [i64, p, p, p, p, p, p, p, p],
        "cvxpnpl_pack_results": [i64, p, p, p, p, p],
        "cvxpnpl_stream_write_value": [p, u64, p], "cvxpnpl_stream_wait_value": [p, u64, p],
        "cvxpnpl_stream_wait_value_bounded": [p, u64, u64, p], "cvxpnpl_stream_wait_gave_up": [p, i32, p],
        "cvxpnpl_score_hypotheses": [i64, p, p, p, C.c_uint32, p, i32, p, p, f64, p, p, p],
        "cvxpnpl_select_best": [i64, p, p, p, p, p, i32, p, p, f64, p, p, p, p, p],
        "cvxpnpl_refit_update": [p, p, p, p, p, i32, p, p, f64, p, p, p, p, p],
        "cvxpnpl_sample_minimal_sets": [i64, i32, p, p, i32, u64, p, p, p, p],
        "cvxpnpl_synth_batch": [i64, i32, i32, f64, u64, p, p, p, p, p, p, p, p],
        "cvxpnpl_pose_errors": [i64, p, p, p, p, p, p, p],
        "cvxpnpl_disambiguate": [i64, p, p, p, p, p, p, p, i32, p, p, p, p],
        "cvxpnpl_workspace_bytes": [i64], "cvxpnpl_set_workspace": [p, size, p], "cvxpnpl_release_workspace": [p, i32],
        "cvxpnpl_calibration_copy": [p, p, i64, i32, p],
        "cvxpnpl_assemble_subsets": [i64, i32, p, p, p, p, p, p, p, p],
        "cvxpnpl_ipm_batch": [i64, p, i32, p, p, p, p, p],
        "cvxpnpl_event_record": [p, p], "cvxpnpl_event_elapsed_ms": [p, p, C.POINTER(C.c_float)], "cvxpnpl_event_destroy": [p],
    }
    for name, types in argtypes.items():
        if name not in _SOLVER_OPTIONAL or hasattr(L, name):
            getattr(L, name).argtypes = types
    L.cvxpnpl_default_opts.restype = L.cvxpnpl_event_destroy.restype = None
    L.cvxpnpl_opts_size.restype = L.cvxpnpl_assemble_large_scratch_bytes.restype = L.cvxpnpl_workspace_bytes.restype = size
    L.cvxpnpl_event_create.restype = p
    if L.cvxpnpl_opts_size() != C.sizeof(Opts):  # the hand-written mirror above and the header must move in lock-step
        raise ImportError(f"cvxpnpl_amd._lib.Opts has {C.sizeof(Opts)} bytes, {LIB_PATH} expects {L.cvxpnpl_opts_size()} (include/cvxpnpl_amd.h)")


def lib():
    """Load libcvxpnpl_amd.so (loudly)."""
    L = _loaded.get(LIB_PATH)  # (every pnp() call comes through here: no message is formatted once the library is loaded)
    if L is not None:
        return L
    return _load(LIB_PATH, EXPORTS, _solver_argtypes,
                 missing=f"{LIB_PATH} is missing: the HIP extension has not been built "
                 "(run `python -c 'import __graft_entry__ as g; g.build()'` or `python -m cvxpnpl_amd.build`). "
                 "cvxpnpl_amd has no CPU fallback.",
                 optional=_SOLVER_OPTIONAL if os.environ.get("CVXPNPL_AMD_LIB") else ())


# the backward pass (include/cvxpnpl_amd_grad.h): a library of its own beside the solver's
GRAD_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_grad.so")
GRAD_EXPORTS = ("cvxpnpl_pose_vjp_batch", "cvxpnpl_pose_vjp_host", "cvxpnpl_grad_last_error")
VJP_OK, VJP_SKIPPED, VJP_SINGULAR, VJP_NONFINITE = 0, 1, 2, 3  # CVXPNPL_VJP_*


def _grad_argtypes(L):
    L.cvxpnpl_pose_vjp_batch.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvxpnpl_pose_vjp_host.argtypes = L.cvxpnpl_pose_vjp_batch.argtypes[:-1] + [C.c_int32]


def grad_lib():
    """Load libcvxpnpl_amd_grad.so (loudly)."""
    return _load(GRAD_LIB_PATH, GRAD_EXPORTS, _grad_argtypes)


# RANSAC over many scenes (include/cvxpnpl_amd_ransac.h): the third library
RANSAC_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac.so")
RANSAC_EXPORTS = ("cvxpnpl_ransac_sample_scenes", "cvxpnpl_ransac_score_scenes", "cvxpnpl_ransac_select_scenes", "cvxpnpl_ransac_assemble_consensus",
                  "cvxpnpl_ransac_refit_update_scenes", "cvxpnpl_ransac_last_error")


def _ransac_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.cvxpnpl_ransac_sample_scenes.argtypes = [i64, i32, p, i64, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_score_scenes.argtypes = [i64, i32, p, i64, p, p, p, C.c_uint32, p, i32, p, p, C.c_double, p, p]
    L.cvxpnpl_ransac_select_scenes.argtypes = [i64, i32, p, i64, p, p, p, p, p, i32, p, p, C.c_double, p, p, p, p, p]
    L.cvxpnpl_ransac_assemble_consensus.argtypes = [i64, p, i64, p, p, p, p, i32, p, p, p, p]
    L.cvxpnpl_ransac_refit_update_scenes.argtypes = [i64, p, i64, p, p, p, p, p, i32, p, p, C.c_double, p, p, p, p, p]


def ransac_lib():
    """Load libcvxpnpl_amd_ransac.so (loudly)."""
    return _load(RANSAC_LIB_PATH, RANSAC_EXPORTS, _ransac_argtypes)


# RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl.h): the fourth library
RANSAC_PNPL_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_pnpl.so")
RANSAC_PNPL_EXPORTS = ("cvxpnpl_ransac_pnpl_sample_assemble", "cvxpnpl_ransac_pnpl_score", "cvxpnpl_ransac_pnpl_select",
                       "cvxpnpl_ransac_pnpl_assemble_consensus", "cvxpnpl_ransac_pnpl_refit_update", "cvxpnpl_ransac_pnpl_last_error")


def _ransac_pnpl_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    scenes = [p, i64, p, i64]  # d_pt_offsets, n_pts, d_ln_offsets, n_lines
    L.cvxpnpl_ransac_pnpl_sample_assemble.argtypes = [i64, i32] + scenes + [p, p, p, p, p, p, i32, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_score.argtypes = [i64, i32] + scenes + [p, p, p, C.c_uint32, p, i32, p, p, p, p, C.c_double, p, p]
    L.cvxpnpl_ransac_pnpl_select.argtypes = [i64, i32] + scenes + [p, p, p, p, p, i32, p, p, p, p, C.c_double, p, p, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_assemble_consensus.argtypes = [i64] + scenes + [p, p, p, p, p, p, p, i32, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_refit_update.argtypes = [i64] + scenes + [p, p, p, p, p, i32, p, p, p, p, C.c_double, p, p, p, p, p, p]


def ransac_pnpl_lib():
    """Load libcvxpnpl_amd_ransac_pnpl.so (loudly)."""
    return _load(RANSAC_PNPL_LIB_PATH, RANSAC_PNPL_EXPORTS, _ransac_pnpl_argtypes)


# reprojection refinement of poses (include/cvxpnpl_amd_refine.h): the fifth library
REFINE_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_refine.so")
REFINE_EXPORTS = ("cvxpnpl_refine_batch", "cvxpnpl_refine_scenes", "cvxpnpl_refine_batch_host", "cvxpnpl_refine_last_error", "cvxpnpl_refine_version")
REFINE_CONVERGED, REFINE_MAXITER, REFINE_SKIPPED, REFINE_SINGULAR, REFINE_BEHIND = 0, 1, 2, 3, 4  # CVXPNPL_REFINE_*


class RefineOpts(C.Structure):
    """cvxpnpl_refine_opts_t"""
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_int32), ("step_tol", C.c_double), ("lambda0", C.c_double), ("sigma_px", C.c_double)]



def _refine_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pose = [p, i32, p, p, p, i64, C.c_uint32, p, p, C.POINTER(RefineOpts)]  # K, K_per, R, t, status, stride, admit, masks, opts
    outs = [p, p, p, p, p, p, p]                                            # R, t, cost, iters, status, n_live, cov
    L.cvxpnpl_refine_batch.argtypes = [i64, i32, p, p, i32, p, p] + pose + outs + [p]
    L.cvxpnpl_refine_batch_host.argtypes = [i64, i32, p, p, i32, p, p] + pose + outs + [i32]
    L.cvxpnpl_refine_scenes.argtypes = [i64, p, i64, p, i64, p, p, p, p] + pose + outs + [p]


def refine_lib():
    """Load libcvxpnpl_amd_refine.so (loudly)."""
    return _load(REFINE_LIB_PATH, REFINE_EXPORTS, _refine_argtypes)


# the backward pass of the refinement (include/cvxpnpl_amd_refine_grad.h): the sixth library
REFINE_GRAD_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_refine_grad.so")
REFINE_GRAD_EXPORTS = ("cvxpnpl_refine_vjp_batch", "cvxpnpl_refine_vjp_scenes", "cvxpnpl_refine_vjp_batch_host", "cvxpnpl_refine_grad_last_error",
                       "cvxpnpl_refine_grad_version")
REFINE_VJP_OK, REFINE_VJP_SKIPPED, REFINE_VJP_SINGULAR, REFINE_VJP_BEHIND = 0, 1, 2, 3  # CVXPNPL_REFINE_VJP_*


def _refine_grad_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pose = [p, i32, p, p, p, i64, C.c_uint32, p, p]  # K, K_per, R, t, refine status, stride, admit, masks
    grads = [p, p, p, p, p, p, p, p]                 # grad_R, grad_t, g_pts_2d, g_pts_3d, g_line_2d, g_line_3d, vjp_status, info
    L.cvxpnpl_refine_vjp_batch.argtypes = [i64, i32, p, p, i32, p, p] + pose + grads + [p]
    L.cvxpnpl_refine_vjp_batch_host.argtypes = [i64, i32, p, p, i32, p, p] + pose + grads + [i32]
    L.cvxpnpl_refine_vjp_scenes.argtypes = [i64, p, i64, p, i64, p, p, p, p] + pose + grads + [p]


def refine_grad_lib():
    """Load libcvxpnpl_amd_refine_grad.so (loudly)."""
    return _load(REFINE_GRAD_LIB_PATH, REFINE_GRAD_EXPORTS, _refine_grad_argtypes)


# the refinement under a robust loss and weights (include/cvxpnpl_amd_refine_robust.h): the seventh library
REFINE_ROBUST_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_refine_robust.so")
REFINE_ROBUST_EXPORTS = ("cvxpnpl_refine_robust_batch", "cvxpnpl_refine_robust_scenes", "cvxpnpl_refine_robust_batch_host",
                         "cvxpnpl_refine_robust_last_error", "cvxpnpl_refine_robust_version")
LOSS_L2, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2  # CVXPNPL_LOSS_*
LOSS_NAMES = {"l2": LOSS_L2, "huber": LOSS_HUBER, "cauchy": LOSS_CAUCHY}


class RefineRobustOpts(C.Structure):
    """cvxpnpl_refine_robust_opts_t"""
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_int32), ("step_tol", C.c_double), ("lambda0", C.c_double), ("loss", C.c_int32),
                ("scale_px", C.c_double)]



def _refine_robust_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pose = [p, i32, p, p, p, i64, C.c_uint32, p, p, p, p, C.POINTER(RefineRobustOpts)]  # K, K_per, R, t, status, stride, admit, masks, weights, opts
    outs = [p, p, p, p, p, p]                                                          # R, t, cost, iters, status, n_live
    L.cvxpnpl_refine_robust_batch.argtypes = [i64, i32, p, p, i32, p, p] + pose + outs + [p, p, p]         # robust_w, n_inlier, stream
    L.cvxpnpl_refine_robust_batch_host.argtypes = [i64, i32, p, p, i32, p, p] + pose + outs + [p, p, i32]  # robust_w, n_inlier, n_threads
    L.cvxpnpl_refine_robust_scenes.argtypes = [i64, p, i64, p, i64, p, p, p, p] + pose + outs + [p, p, p, p]  # robust_w_pts, robust_w_lines, n_inlier, stream


def refine_robust_lib():
    """Load libcvxpnpl_amd_refine_robust.so (loudly)."""
    return _load(REFINE_ROBUST_LIB_PATH, REFINE_ROBUST_EXPORTS, _refine_robust_argtypes)


# the backward pass of the robust refinement (include/cvxpnpl_amd_refine_robust_grad.h): the eighth library
REFINE_ROBUST_GRAD_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_refine_robust_grad.so")
REFINE_ROBUST_GRAD_EXPORTS = ("cvxpnpl_refine_robust_vjp_batch", "cvxpnpl_refine_robust_vjp_scenes", "cvxpnpl_refine_robust_vjp_batch_host",
                              "cvxpnpl_refine_robust_grad_last_error", "cvxpnpl_refine_robust_grad_version")


def _refine_robust_grad_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pose = [p, i32, p, p, p, i64, C.c_uint32, i32, C.c_double, p, p, p, p]  # K, K_per, R, t, refine status, stride, admit, loss, scale_px, masks, weights
    grads = [p, p, p, p, p, p, p, p, p, p]  # grad_R, grad_t, g_pts_2d, g_pts_3d, g_line_2d, g_line_3d, g_w_pts, g_w_lines, vjp_status, info
    L.cvxpnpl_refine_robust_vjp_batch.argtypes = [i64, i32, p, p, i32, p, p] + pose + grads + [p]
    L.cvxpnpl_refine_robust_vjp_batch_host.argtypes = [i64, i32, p, p, i32, p, p] + pose + grads + [i32]
    L.cvxpnpl_refine_robust_vjp_scenes.argtypes = [i64, p, i64, p, i64, p, p, p, p] + pose + grads + [p]


def refine_robust_grad_lib():
    """Load libcvxpnpl_amd_refine_robust_grad.so (loudly)."""
    return _load(REFINE_ROBUST_GRAD_LIB_PATH, REFINE_ROBUST_GRAD_EXPORTS, _refine_robust_grad_argtypes)


# adaptive RANSAC, a hypothesis budget per scene solved in rounds (include/cvxpnpl_amd_ransac_adaptive.h): the ninth library
RANSAC_ADAPTIVE_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_adaptive.so")
RANSAC_ADAPTIVE_EXPORTS = ("cvxpnpl_ransac_adaptive_init", "cvxpnpl_ransac_adaptive_sample", "cvxpnpl_ransac_adaptive_score",
                           "cvxpnpl_ransac_adaptive_update", "cvxpnpl_ransac_adaptive_compact", "cvxpnpl_ransac_adaptive_needed_host",
                           "cvxpnpl_ransac_adaptive_last_error")


def _ransac_adaptive_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.cvxpnpl_ransac_adaptive_init.argtypes = [i64, p, p, p, p, p, p]
    L.cvxpnpl_ransac_adaptive_sample.argtypes = [i64, i64, p, i32, i32, i32, p, i64, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_adaptive_score.argtypes = [i64, i64, p, i32, p, i64, p, p, p, C.c_uint32, p, i32, p, p, C.c_double, p, p]
    L.cvxpnpl_ransac_adaptive_update.argtypes = [i64, i64, p, i32, i32, i32, C.c_double, p, i64, p, p, p, p, p, i32, p, p, C.c_double,
                                                 p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_adaptive_compact.argtypes = [i64, i64, p, p, p, p, p]
    L.cvxpnpl_ransac_adaptive_needed_host.argtypes = [i32, i32, C.c_double]
    L.cvxpnpl_ransac_adaptive_needed_host.restype = C.c_double


def ransac_adaptive_lib():
    """Load libcvxpnpl_amd_ransac_adaptive.so (loudly)."""
    return _load(RANSAC_ADAPTIVE_LIB_PATH, RANSAC_ADAPTIVE_EXPORTS, _ransac_adaptive_argtypes)


# guided RANSAC, minimal sets drawn from the best-ranked correspondences first (include/cvxpnpl_amd_ransac_guided.h): the tenth library
RANSAC_GUIDED_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_guided.so")
RANSAC_GUIDED_EXPORTS = ("cvxpnpl_ransac_guided_rank", "cvxpnpl_ransac_guided_sample", "cvxpnpl_ransac_guided_sample_active",
                         "cvxpnpl_ransac_guided_rank_host", "cvxpnpl_ransac_guided_pool_host", "cvxpnpl_ransac_guided_last_error")


def _ransac_guided_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.cvxpnpl_ransac_guided_rank.argtypes = [i64, p, i64, i32, p, p, p]
    L.cvxpnpl_ransac_guided_sample.argtypes = [i64, i32, i32, p, i64, p, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_guided_sample_active.argtypes = [i64, i64, p, i32, i32, i32, i32, p, i64, p, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_guided_rank_host.argtypes = [i64, p, i64, p, p, i32]
    L.cvxpnpl_ransac_guided_pool_host.argtypes = [i32, i32, i32]
    L.cvxpnpl_ransac_guided_pool_host.restype = i32


def ransac_guided_lib():
    """Load libcvxpnpl_amd_ransac_guided.so (loudly)."""
    return _load(RANSAC_GUIDED_LIB_PATH, RANSAC_GUIDED_EXPORTS, _ransac_guided_argtypes)


# adaptive and guided RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl_adaptive.h): the eleventh library
RANSAC_PNPL_ADAPTIVE_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_pnpl_adaptive.so")
RANSAC_PNPL_ADAPTIVE_EXPORTS = ("cvxpnpl_ransac_pnpl_adaptive_sample_assemble", "cvxpnpl_ransac_pnpl_adaptive_score",
                                "cvxpnpl_ransac_pnpl_adaptive_update", "cvxpnpl_ransac_pnpl_adaptive_last_error")


def _ransac_pnpl_adaptive_argtypes(L):
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    scenes = [p, i64, p, i64]  # d_pt_offsets, n_pts, d_ln_offsets, n_lines
    L.cvxpnpl_ransac_pnpl_adaptive_sample_assemble.argtypes = [i64, i64, p, i32, i32, i32, i32] + scenes + [p, p, p, p, p, p, p, i32, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_adaptive_score.argtypes = [i64, i64, p, i32] + scenes + [p, p, p, C.c_uint32, p, i32, p, p, p, p, C.c_double, p, p]
    L.cvxpnpl_ransac_pnpl_adaptive_update.argtypes = [i64, i64, p, i32, i32, i32, C.c_double] + scenes + [p, p, p, p, p, i32, p, p, p, p, C.c_double,
                                                                                                            p, p, p, p, p, p, p, p, p]


def ransac_pnpl_adaptive_lib():
    """Load libcvxpnpl_amd_ransac_pnpl_adaptive.so (loudly)."""
    return _load(RANSAC_PNPL_ADAPTIVE_LIB_PATH, RANSAC_PNPL_ADAPTIVE_EXPORTS, _ransac_pnpl_adaptive_argtypes)


# the robust refinement at a scale per problem, its scale estimate and its sandwich covariance (include/cvxpnpl_amd_refine_robust_auto.h):
# the twelfth library
REFINE_ROBUST_AUTO_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_refine_robust_auto.so")
REFINE_ROBUST_AUTO_EXPORTS = ("cvxpnpl_robust_scale_batch", "cvxpnpl_robust_scale_scenes", "cvxpnpl_robust_scale_batch_host",
                              "cvxpnpl_refine_robust_pp_batch", "cvxpnpl_refine_robust_pp_scenes", "cvxpnpl_refine_robust_pp_batch_host",
                              "cvxpnpl_robust_cov_batch", "cvxpnpl_robust_cov_scenes", "cvxpnpl_robust_cov_batch_host",
                              "cvxpnpl_refine_robust_auto_last_error", "cvxpnpl_refine_robust_auto_version")
RefineRobustAutoOpts = RefineRobustOpts  # the loop at a scale per problem takes cvxpnpl_refine_robust_opts_t as it is


def _refine_robust_auto_argtypes(L):
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    batch, scenes = [i64, i32, p, p, i32, p, p], [i64, p, i64, p, i64, p, p, p, p]
    pose = [p, i32, p, p, p, i64, C.c_uint32, p, p, p, p]  # K, K_per, R, t, status, stride, admit, masks, weights
    loop = pose + [p, C.POINTER(RefineRobustAutoOpts)] + [p, p, p, p, p, p]  # scale_px [n], opts; R, t, cost, iters, status, n_live
    cov = [p, i32, p, p, p, p, p, p, p, i32, f64, p, p, p]  # K, K_per, R, t, status, masks, weights, loss, scale_px, scale_px [n], cov, cov_status
    L.cvxpnpl_robust_scale_batch.argtypes = batch + pose + [p, p, p, p, p, p]          # sigma, med_sq, n_live, status, sq, stream
    L.cvxpnpl_robust_scale_batch_host.argtypes = batch + pose + [p, p, p, p, p, i32]   # ..., n_threads
    L.cvxpnpl_robust_scale_scenes.argtypes = scenes + pose + [p, p, p, p, p, p, p]     # sigma, med_sq, n_live, status, sq_pts, sq_lines, stream
    L.cvxpnpl_refine_robust_pp_batch.argtypes = batch + loop + [p, p, p]               # robust_w, n_inlier, stream
    L.cvxpnpl_refine_robust_pp_batch_host.argtypes = batch + loop + [p, p, i32]        # robust_w, n_inlier, n_threads
    L.cvxpnpl_refine_robust_pp_scenes.argtypes = scenes + loop + [p, p, p, p]          # robust_w_pts, robust_w_lines, n_inlier, stream
    L.cvxpnpl_robust_cov_batch.argtypes = batch + cov + [p]
    L.cvxpnpl_robust_cov_batch_host.argtypes = batch + cov + [i32]
    L.cvxpnpl_robust_cov_scenes.argtypes = scenes + cov + [p]


def refine_robust_auto_lib():
    """Load libcvxpnpl_amd_refine_robust_auto.so (loudly)."""
    return _load(REFINE_ROBUST_AUTO_LIB_PATH, REFINE_ROBUST_AUTO_EXPORTS, _refine_robust_auto_argtypes)


# MSAC scoring for RANSAC over many scenes (include/cvxpnpl_amd_ransac_msac.h): the thirteenth library
RANSAC_MSAC_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_msac.so")
RANSAC_MSAC_EXPORTS = ("cvxpnpl_ransac_msac_score_scenes", "cvxpnpl_ransac_msac_score_active", "cvxpnpl_ransac_msac_select_scenes",
                       "cvxpnpl_ransac_msac_init", "cvxpnpl_ransac_msac_update", "cvxpnpl_ransac_msac_score_host", "cvxpnpl_ransac_msac_last_error")


def _ransac_msac_argtypes(L):
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.cvxpnpl_ransac_msac_score_scenes.argtypes = [i64, i32, p, i64, p, p, p, C.c_uint32, p, i32, p, p, f64, p, p, p]
    L.cvxpnpl_ransac_msac_score_active.argtypes = [i64, i64, p, i32, p, i64, p, p, p, C.c_uint32, p, i32, p, p, f64, p, p, p]
    L.cvxpnpl_ransac_msac_select_scenes.argtypes = [i64, i32, p, i64, p, p, p, p, p, i32, p, p, f64, p, p, p, p, p, p]
    L.cvxpnpl_ransac_msac_init.argtypes = [i64, p, p]
    L.cvxpnpl_ransac_msac_update.argtypes = [i64, i64, p, i32, i32, i32, f64, p, i64, p, p, p, p, p, p, i32, p, p, f64,
                                             p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_msac_score_host.argtypes = [i64, i32, p, i64, p, p, p, C.c_uint32, p, i32, p, p, f64, p, p, i32]


def ransac_msac_lib():
    """Load libcvxpnpl_amd_ransac_msac.so (loudly)."""
    return _load(RANSAC_MSAC_LIB_PATH, RANSAC_MSAC_EXPORTS, _ransac_msac_argtypes)


# local optimisation in adaptive RANSAC (include/cvxpnpl_amd_ransac_lo.h): the fourteenth library
RANSAC_LO_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_lo.so")
RANSAC_LO_EXPORTS = ("cvxpnpl_ransac_lo_init", "cvxpnpl_ransac_lo_assemble", "cvxpnpl_ransac_lo_update", "cvxpnpl_ransac_lo_assemble_host",
                     "cvxpnpl_ransac_lo_last_error")


def _ransac_lo_argtypes(L):
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.cvxpnpl_ransac_lo_init.argtypes = [i64, p, p]
    L.cvxpnpl_ransac_lo_assemble.argtypes = [i64, i64, p, p, i64, p, p, p, p, p, i32, f64, p, p, p, p]
    L.cvxpnpl_ransac_lo_update.argtypes = [i64, i64, p, i32, f64, p, i64, p, p, p, p, p, i32, p, p, f64, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_lo_assemble_host.argtypes = [i64, i64, p, p, i64, p, p, p, p, p, i32, f64, p, p, p, i32]


def ransac_lo_lib():
    """Load libcvxpnpl_amd_ransac_lo.so (loudly)."""
    return _load(RANSAC_LO_LIB_PATH, RANSAC_LO_EXPORTS, _ransac_lo_argtypes)


# local optimisation in adaptive RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl_lo.h): the fifteenth library
RANSAC_PNPL_LO_LIB_PATH = os.path.join(_HERE, "libcvxpnpl_amd_ransac_pnpl_lo.so")
RANSAC_PNPL_LO_EXPORTS = ("cvxpnpl_ransac_pnpl_lo_assemble", "cvxpnpl_ransac_pnpl_lo_update", "cvxpnpl_ransac_pnpl_lo_assemble_host",
                          "cvxpnpl_ransac_pnpl_lo_last_error")


def _ransac_pnpl_lo_argtypes(L):
    i64, i32, f64, p = C.c_int64, C.c_int32, C.c_double, C.c_void_p
    scenes, data = [p, i64, p, i64], [p, p, p, p]  # d_pt_offsets, n_pts, d_ln_offsets, n_lines; d_pts_2d, d_pts_3d, d_line_2d, d_line_3d
    L.cvxpnpl_ransac_pnpl_lo_assemble.argtypes = [i64, i64, p] + scenes + data + [p, p, p, i32, f64, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_lo_update.argtypes = [i64, i64, p, i32, f64] + scenes + [p, p, p, p, p, i32] + data + [f64, p, p, p, p, p, p, p, p, p, p]
    L.cvxpnpl_ransac_pnpl_lo_assemble_host.argtypes = [i64, i64, p] + scenes + data + [p, p, p, i32, f64, p, p, p, i32]


def ransac_pnpl_lo_lib():
    """Load libcvxpnpl_amd_ransac_pnpl_lo.so (loudly)."""
    return _load(RANSAC_PNPL_LO_LIB_PATH, RANSAC_PNPL_LO_EXPORTS, _ransac_pnpl_lo_argtypes)


def default_opts(**overrides):
    o = Opts()
    lib().cvxpnpl_default_opts(C.byref(o))
    for k, v in overrides.items():
        if v is None:
            continue
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k!r}")
        setattr(o, k, v)
    return o


def last_error():
    return lib().cvxpnpl_last_error().decode()
