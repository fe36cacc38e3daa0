"""Build the HIP shared library in-tree:  python -m cvxpnpl_amd.build"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "cvxpnpl_hip.hip")
HOST_SRC = os.path.join(HERE, "csrc", "host_recover.cpp")
LANE_SRC = os.path.join(HERE, "csrc", "lane_kernel.hip")  # solve_lane2_kernel: a translation unit of its own (see its header)
OUT = os.path.join(HERE, "libcvxpnpl_amd.so")
ENTRY_ERROR_H = os.path.join(HERE, "csrc", "entry_error.h")  # the error text of every library's entry points
SOLVER_ENTRY_HEADERS = [os.path.join(HERE, "csrc", "solver_entry.h"), ENTRY_ERROR_H]  # what the solver's and the pose VJP's entry files share
DEPS = [SRC, HOST_SRC, LANE_SRC, *SOLVER_ENTRY_HEADERS, os.path.join(HERE, "csrc", "batch_args.h"), os.path.join(HERE, "csrc", "launch_plan.h"), os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
        os.path.join(HERE, "csrc", "wave_kernel.h"), os.path.join(HERE, "csrc", "quad_kernel.h"), os.path.join(HERE, "csrc", "score_kernel.h"), os.path.join(HERE, "csrc", "assemble_kernel.h"), os.path.join(HERE, "csrc", "synth_kernel.h"), os.path.join(HERE, "csrc", "recover_core.h"), os.path.join(HERE, "csrc", "recover_kernel.h"),
        os.path.join(HERE, "csrc", "ipm_core.h"), os.path.join(HERE, "csrc", "ipm_wave.h"), os.path.join(HERE, "csrc", "ipm_quad.h"), os.path.join(HERE, "csrc", "lane_core.h"),
        os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd.h")]


RANSAC_ENTRY_DEPS = [os.path.join(HERE, "csrc", "ransac_entry.h"), ENTRY_ERROR_H]  # what the nine RANSAC entry files share


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


RESOURCES = os.path.join(HERE, "libcvxpnpl_amd.resources.txt")  # the compiler's kernel-resource remarks of the build that made OUT


def compile_cmd(out=OUT):
    srcs = [SRC, LANE_SRC] + ([HOST_SRC] if os.path.exists(HOST_SRC) else [])
    # -enable-ipra=0: the one non-inlined device function (cvxw::coop_ipm) is called from the rescue kernel only; with
    # inter-procedural register allocation the CALLER's first-order loop around it came out 40 % slower (profiles/r02/ipm_clock.jsonl)
    # -Rpass-analysis=kernel-resource-usage: registers / scratch / occupancy / LDS of every kernel, kept beside the library
    # (RESOURCES) and held against tests/golden/kernel_resources.json by tests/test_kernel_resources.py
    return [hipcc(), "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
            "-mllvm", "-enable-ipra=0", "-o", out] + srcs


# the backward pass of the solves (include/cvxpnpl_amd_grad.h): a library of its own, with its own resource remarks
GRAD_SRC = os.path.join(HERE, "csrc", "grad_hip.hip")
GRAD_HOST_SRC = os.path.join(HERE, "csrc", "host_vjp.cpp")
GRAD_OUT = os.path.join(HERE, "libcvxpnpl_amd_grad.so")
GRAD_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_grad.resources.txt")
GRAD_DEPS = [GRAD_SRC, GRAD_HOST_SRC, *SOLVER_ENTRY_HEADERS, os.path.join(HERE, "csrc", "vjp_core.h"), os.path.join(HERE, "csrc", "vjp_kernel.h"), os.path.join(HERE, "csrc", "solver_core.h"),
             os.path.join(HERE, "csrc", "host_pool.h"),
             os.path.join(HERE, "csrc", "problem_io.h"), os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_grad.h")]


def grad_compile_cmd(out=GRAD_OUT):
    return [hipcc(), "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
            "-o", out, GRAD_SRC, GRAD_HOST_SRC]


# RANSAC over many scenes (include/cvxpnpl_amd_ransac.h): the third library, with its own resource remarks
RANSAC_SRC = os.path.join(HERE, "csrc", "ransac_hip.hip")
RANSAC_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac.so")
RANSAC_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac.resources.txt")
RANSAC_DEPS = [RANSAC_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_kernel.h"), os.path.join(HERE, "csrc", "ransac_assemble_core.h"), os.path.join(HERE, "csrc", "ransac_common.h"), os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
               os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac.h")]


def ransac_compile_cmd(out=RANSAC_OUT):
    return [hipcc(), "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
            "-o", out, RANSAC_SRC]


# RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl.h): the fourth library, same flags as the third
RANSAC_PNPL_SRC = os.path.join(HERE, "csrc", "ransac_pnpl_hip.hip")
RANSAC_PNPL_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl.so")
RANSAC_PNPL_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl.resources.txt")
RANSAC_PNPL_DEPS = [RANSAC_PNPL_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_pnpl_kernel.h"), os.path.join(HERE, "csrc", "ransac_pnpl_common.h"),
                    os.path.join(HERE, "csrc", "ransac_assemble_core.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                    os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                    os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_pnpl.h")]


def ransac_pnpl_compile_cmd(out=RANSAC_PNPL_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_PNPL_SRC]


# reprojection refinement of poses (include/cvxpnpl_amd_refine.h): the fifth library, device and host entry points as in the second
REFINE_SRC = os.path.join(HERE, "csrc", "refine_hip.hip")
REFINE_HOST_SRC = os.path.join(HERE, "csrc", "host_refine.cpp")
REFINE_OUT = os.path.join(HERE, "libcvxpnpl_amd_refine.so")
REFINE_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_refine.resources.txt")
REFINE_DEPS = [REFINE_SRC, REFINE_HOST_SRC, os.path.join(HERE, "csrc", "refine_core.h"), os.path.join(HERE, "csrc", "refine_kernel.h"), os.path.join(HERE, "csrc", "refine_lanes.h"), os.path.join(HERE, "csrc", "refine_view.h"),
               os.path.join(HERE, "csrc", "ransac_common.h"), os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
               os.path.join(HERE, "csrc", "refine_entry.h"), ENTRY_ERROR_H, os.path.join(HERE, "csrc", "host_pool.h"),
               os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine.h")]


def refine_compile_cmd(out=REFINE_OUT):
    return grad_compile_cmd(out)[:-2] + [REFINE_SRC, REFINE_HOST_SRC]


# the backward pass of the refinement (include/cvxpnpl_amd_refine_grad.h): the sixth library, the flags of the second and the fifth
REFINE_GRAD_SRC = os.path.join(HERE, "csrc", "refine_grad_hip.hip")
REFINE_GRAD_HOST_SRC = os.path.join(HERE, "csrc", "host_refine_vjp.cpp")
REFINE_GRAD_OUT = os.path.join(HERE, "libcvxpnpl_amd_refine_grad.so")
REFINE_GRAD_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_refine_grad.resources.txt")
REFINE_GRAD_DEPS = [REFINE_GRAD_SRC, REFINE_GRAD_HOST_SRC, os.path.join(HERE, "csrc", "refine_vjp_core.h"), os.path.join(HERE, "csrc", "refine_vjp_kernel.h"),
                    os.path.join(HERE, "csrc", "refine_core.h"), os.path.join(HERE, "csrc", "refine_lanes.h"), os.path.join(HERE, "csrc", "refine_view.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                    os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                    os.path.join(HERE, "csrc", "refine_entry.h"), ENTRY_ERROR_H, os.path.join(HERE, "csrc", "host_pool.h"),
                    os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine_grad.h")]


def refine_grad_compile_cmd(out=REFINE_GRAD_OUT):
    return grad_compile_cmd(out)[:-2] + [REFINE_GRAD_SRC, REFINE_GRAD_HOST_SRC]


# the refinement under a robust loss and weights (include/cvxpnpl_amd_refine_robust.h): the seventh library, the flags of the fifth and sixth
REFINE_ROBUST_SRC = os.path.join(HERE, "csrc", "refine_robust_hip.hip")
REFINE_ROBUST_HOST_SRC = os.path.join(HERE, "csrc", "host_refine_robust.cpp")
REFINE_ROBUST_OUT = os.path.join(HERE, "libcvxpnpl_amd_refine_robust.so")
REFINE_ROBUST_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_refine_robust.resources.txt")
REFINE_ROBUST_DEPS = [REFINE_ROBUST_SRC, REFINE_ROBUST_HOST_SRC, os.path.join(HERE, "csrc", "refine_robust_core.h"), os.path.join(HERE, "csrc", "refine_robust_kernel.h"),
                      os.path.join(HERE, "csrc", "refine_core.h"), os.path.join(HERE, "csrc", "refine_lanes.h"), os.path.join(HERE, "csrc", "refine_view.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                      os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                      os.path.join(HERE, "csrc", "refine_entry.h"), ENTRY_ERROR_H, os.path.join(HERE, "csrc", "host_pool.h"),
                      os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine_robust.h")]


def refine_robust_compile_cmd(out=REFINE_ROBUST_OUT):
    return grad_compile_cmd(out)[:-2] + [REFINE_ROBUST_SRC, REFINE_ROBUST_HOST_SRC]


# the backward pass of the robust refinement (include/cvxpnpl_amd_refine_robust_grad.h): the eighth library, the flags of the fifth to seventh
REFINE_ROBUST_GRAD_SRC = os.path.join(HERE, "csrc", "refine_robust_grad_hip.hip")
REFINE_ROBUST_GRAD_HOST_SRC = os.path.join(HERE, "csrc", "host_refine_robust_vjp.cpp")
REFINE_ROBUST_GRAD_OUT = os.path.join(HERE, "libcvxpnpl_amd_refine_robust_grad.so")
REFINE_ROBUST_GRAD_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_refine_robust_grad.resources.txt")
REFINE_ROBUST_GRAD_DEPS = [REFINE_ROBUST_GRAD_SRC, REFINE_ROBUST_GRAD_HOST_SRC, os.path.join(HERE, "csrc", "refine_robust_vjp_core.h"),
                           os.path.join(HERE, "csrc", "refine_robust_vjp_kernel.h"), os.path.join(HERE, "csrc", "refine_robust_core.h"),
                           os.path.join(HERE, "csrc", "refine_robust_kernel.h"), os.path.join(HERE, "csrc", "refine_vjp_core.h"),
                           os.path.join(HERE, "csrc", "refine_core.h"), os.path.join(HERE, "csrc", "refine_lanes.h"), os.path.join(HERE, "csrc", "refine_view.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                           os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                           os.path.join(HERE, "csrc", "refine_entry.h"), ENTRY_ERROR_H, os.path.join(HERE, "csrc", "host_pool.h"),
                           os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine_robust_grad.h")]


def refine_robust_grad_compile_cmd(out=REFINE_ROBUST_GRAD_OUT):
    return grad_compile_cmd(out)[:-2] + [REFINE_ROBUST_GRAD_SRC, REFINE_ROBUST_GRAD_HOST_SRC]


# adaptive RANSAC, a hypothesis budget per scene solved in rounds (include/cvxpnpl_amd_ransac_adaptive.h): the ninth library, the flags of
# the third
RANSAC_ADAPTIVE_SRC = os.path.join(HERE, "csrc", "ransac_adaptive_hip.hip")
RANSAC_ADAPTIVE_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_adaptive.so")
RANSAC_ADAPTIVE_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_adaptive.resources.txt")
RANSAC_ADAPTIVE_DEPS = [RANSAC_ADAPTIVE_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_adaptive_kernel.h"), os.path.join(HERE, "csrc", "ransac_adaptive_core.h"),
                        os.path.join(HERE, "csrc", "ransac_common.h"), os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_adaptive.h")]


def ransac_adaptive_compile_cmd(out=RANSAC_ADAPTIVE_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_ADAPTIVE_SRC]


# guided RANSAC, minimal sets drawn from the best-ranked correspondences first (include/cvxpnpl_amd_ransac_guided.h): the tenth library, the
# flags of the third
RANSAC_GUIDED_SRC = os.path.join(HERE, "csrc", "ransac_guided_hip.hip")
RANSAC_GUIDED_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_guided.so")
RANSAC_GUIDED_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_guided.resources.txt")
RANSAC_GUIDED_DEPS = [RANSAC_GUIDED_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_guided_kernel.h"), os.path.join(HERE, "csrc", "ransac_guided_core.h"),
                      os.path.join(HERE, "csrc", "ransac_common.h"), os.path.join(HERE, "csrc", "host_pool.h"),
                      os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_guided.h")]


def ransac_guided_compile_cmd(out=RANSAC_GUIDED_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_GUIDED_SRC]


# adaptive and guided RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl_adaptive.h): the eleventh library, the flags of the
# third
RANSAC_PNPL_ADAPTIVE_SRC = os.path.join(HERE, "csrc", "ransac_pnpl_adaptive_hip.hip")
RANSAC_PNPL_ADAPTIVE_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl_adaptive.so")
RANSAC_PNPL_ADAPTIVE_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl_adaptive.resources.txt")
RANSAC_PNPL_ADAPTIVE_DEPS = [RANSAC_PNPL_ADAPTIVE_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_pnpl_adaptive_kernel.h"),
                             os.path.join(HERE, "csrc", "ransac_pnpl_common.h"), os.path.join(HERE, "csrc", "ransac_adaptive_core.h"),
                             os.path.join(HERE, "csrc", "ransac_guided_core.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                             os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                             os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_pnpl_adaptive.h")]


def ransac_pnpl_adaptive_compile_cmd(out=RANSAC_PNPL_ADAPTIVE_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_PNPL_ADAPTIVE_SRC]


# the robust refinement at a scale per problem: a scale from the median squared residual, the loop at that scale and the sandwich covariance
# (include/cvxpnpl_amd_refine_robust_auto.h): the twelfth library, the flags of the fifth to eighth
REFINE_ROBUST_AUTO_SRC = os.path.join(HERE, "csrc", "refine_robust_auto_hip.hip")
REFINE_ROBUST_AUTO_HOST_SRC = os.path.join(HERE, "csrc", "host_refine_robust_auto.cpp")
REFINE_ROBUST_AUTO_OUT = os.path.join(HERE, "libcvxpnpl_amd_refine_robust_auto.so")
REFINE_ROBUST_AUTO_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_refine_robust_auto.resources.txt")
REFINE_ROBUST_AUTO_DEPS = [REFINE_ROBUST_AUTO_SRC, REFINE_ROBUST_AUTO_HOST_SRC, os.path.join(HERE, "csrc", "refine_robust_auto_core.h"),
                           os.path.join(HERE, "csrc", "refine_robust_auto_kernel.h"), os.path.join(HERE, "csrc", "refine_robust_vjp_core.h"),
                           os.path.join(HERE, "csrc", "refine_robust_core.h"), os.path.join(HERE, "csrc", "refine_robust_kernel.h"),
                           os.path.join(HERE, "csrc", "refine_vjp_core.h"), os.path.join(HERE, "csrc", "refine_core.h"),
                           os.path.join(HERE, "csrc", "refine_lanes.h"), os.path.join(HERE, "csrc", "refine_view.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                           os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                           os.path.join(HERE, "csrc", "refine_entry.h"), ENTRY_ERROR_H, os.path.join(HERE, "csrc", "host_pool.h"),
                           os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine_robust.h"),
                           os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_refine_robust_auto.h")]


def refine_robust_auto_compile_cmd(out=REFINE_ROBUST_AUTO_OUT):
    return grad_compile_cmd(out)[:-2] + [REFINE_ROBUST_AUTO_SRC, REFINE_ROBUST_AUTO_HOST_SRC]


# MSAC scoring for RANSAC over many scenes, the hypothesis selected by its truncated quadratic cost (include/cvxpnpl_amd_ransac_msac.h): the
# thirteenth library, the flags of the third.  (Named apart from the twelve pairs above, whose set tests/test_build_deps.py pins;
# tests/test_ransac_msac_library.py holds this list against the include closure of its source.)
RANSAC_MSAC_SRC = os.path.join(HERE, "csrc", "ransac_msac_hip.hip")
RANSAC_MSAC_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_msac.so")
RANSAC_MSAC_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_msac.resources.txt")
RANSAC_MSAC_SOURCES = [RANSAC_MSAC_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_msac_kernel.h"), os.path.join(HERE, "csrc", "ransac_msac_core.h"),
                       os.path.join(HERE, "csrc", "ransac_adaptive_core.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                       os.path.join(HERE, "csrc", "host_pool.h"), os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_msac.h")]


def ransac_msac_command(out=RANSAC_MSAC_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_MSAC_SRC]


# local optimisation in adaptive RANSAC, the running best refitted every round (include/cvxpnpl_amd_ransac_lo.h): the fourteenth library,
# the flags of the third.  (Named as the thirteenth pair is, apart from the twelve tests/test_build_deps.py pins;
# tests/test_ransac_lo_library.py holds this list against the include closure of its source.)
RANSAC_LO_SRC = os.path.join(HERE, "csrc", "ransac_lo_hip.hip")
RANSAC_LO_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_lo.so")
RANSAC_LO_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_lo.resources.txt")
RANSAC_LO_SOURCES = [RANSAC_LO_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_lo_kernel.h"), os.path.join(HERE, "csrc", "ransac_lo_core.h"),
                     os.path.join(HERE, "csrc", "ransac_assemble_core.h"), os.path.join(HERE, "csrc", "ransac_adaptive_core.h"), os.path.join(HERE, "csrc", "ransac_common.h"),
                     os.path.join(HERE, "csrc", "solver_core.h"), os.path.join(HERE, "csrc", "problem_io.h"),
                     os.path.join(HERE, "csrc", "host_pool.h"), os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_lo.h")]


def ransac_lo_command(out=RANSAC_LO_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_LO_SRC]


# local optimisation in adaptive RANSAC over points and lines (include/cvxpnpl_amd_ransac_pnpl_lo.h): the fifteenth library, the flags of the
# third.  (Named as the thirteenth and fourteenth pairs are; tests/test_ransac_pnpl_lo_library.py holds this list against the include
# closure of its source.)
RANSAC_PNPL_LO_SRC = os.path.join(HERE, "csrc", "ransac_pnpl_lo_hip.hip")
RANSAC_PNPL_LO_OUT = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl_lo.so")
RANSAC_PNPL_LO_RESOURCES = os.path.join(HERE, "libcvxpnpl_amd_ransac_pnpl_lo.resources.txt")
RANSAC_PNPL_LO_SOURCES = [RANSAC_PNPL_LO_SRC, *RANSAC_ENTRY_DEPS, os.path.join(HERE, "csrc", "ransac_pnpl_lo_kernel.h"),
                          os.path.join(HERE, "csrc", "ransac_pnpl_lo_core.h"), os.path.join(HERE, "csrc", "ransac_lo_core.h"), os.path.join(HERE, "csrc", "ransac_assemble_core.h"),
                          os.path.join(HERE, "csrc", "ransac_pnpl_common.h"), os.path.join(HERE, "csrc", "ransac_adaptive_core.h"),
                          os.path.join(HERE, "csrc", "ransac_common.h"), os.path.join(HERE, "csrc", "solver_core.h"),
                          os.path.join(HERE, "csrc", "problem_io.h"), os.path.join(HERE, "csrc", "host_pool.h"),
                          os.path.join(os.path.dirname(HERE), "include", "cvxpnpl_amd_ransac_pnpl_lo.h")]


def ransac_pnpl_lo_command(out=RANSAC_PNPL_LO_OUT):
    return ransac_compile_cmd(out)[:-1] + [RANSAC_PNPL_LO_SRC]


def _build_one(out, resources, deps, cmd, force, verbose):
    deps = [d for d in deps if os.path.exists(d)]
    fresh = os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps)
    if not force and fresh and os.path.exists(resources) and os.path.getmtime(resources) >= os.path.getmtime(out):
        return out
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-8000:])
        raise subprocess.CalledProcessError(r.returncode, cmd)
    with open(resources, "w") as f:
        f.write(r.stderr)
    if verbose:
        sys.stderr.write(r.stderr)
    return out


def build_grad(force=False, verbose=False):
    return _build_one(GRAD_OUT, GRAD_RESOURCES, GRAD_DEPS, grad_compile_cmd(), force, verbose)


def build_ransac(force=False, verbose=False):
    return _build_one(RANSAC_OUT, RANSAC_RESOURCES, RANSAC_DEPS, ransac_compile_cmd(), force, verbose)


def build_ransac_pnpl(force=False, verbose=False):
    return _build_one(RANSAC_PNPL_OUT, RANSAC_PNPL_RESOURCES, RANSAC_PNPL_DEPS, ransac_pnpl_compile_cmd(), force, verbose)


def build_refine(force=False, verbose=False):
    return _build_one(REFINE_OUT, REFINE_RESOURCES, REFINE_DEPS, refine_compile_cmd(), force, verbose)


def build_refine_grad(force=False, verbose=False):
    return _build_one(REFINE_GRAD_OUT, REFINE_GRAD_RESOURCES, REFINE_GRAD_DEPS, refine_grad_compile_cmd(), force, verbose)


def build_refine_robust(force=False, verbose=False):
    return _build_one(REFINE_ROBUST_OUT, REFINE_ROBUST_RESOURCES, REFINE_ROBUST_DEPS, refine_robust_compile_cmd(), force, verbose)


def build_refine_robust_grad(force=False, verbose=False):
    return _build_one(REFINE_ROBUST_GRAD_OUT, REFINE_ROBUST_GRAD_RESOURCES, REFINE_ROBUST_GRAD_DEPS, refine_robust_grad_compile_cmd(), force, verbose)


def build_ransac_adaptive(force=False, verbose=False):
    return _build_one(RANSAC_ADAPTIVE_OUT, RANSAC_ADAPTIVE_RESOURCES, RANSAC_ADAPTIVE_DEPS, ransac_adaptive_compile_cmd(), force, verbose)


def build_ransac_guided(force=False, verbose=False):
    return _build_one(RANSAC_GUIDED_OUT, RANSAC_GUIDED_RESOURCES, RANSAC_GUIDED_DEPS, ransac_guided_compile_cmd(), force, verbose)


def build_ransac_pnpl_adaptive(force=False, verbose=False):
    return _build_one(RANSAC_PNPL_ADAPTIVE_OUT, RANSAC_PNPL_ADAPTIVE_RESOURCES, RANSAC_PNPL_ADAPTIVE_DEPS, ransac_pnpl_adaptive_compile_cmd(), force, verbose)


def build_refine_robust_auto(force=False, verbose=False):
    return _build_one(REFINE_ROBUST_AUTO_OUT, REFINE_ROBUST_AUTO_RESOURCES, REFINE_ROBUST_AUTO_DEPS, refine_robust_auto_compile_cmd(), force, verbose)


def build_ransac_msac(force=False, verbose=False):
    return _build_one(RANSAC_MSAC_OUT, RANSAC_MSAC_RESOURCES, RANSAC_MSAC_SOURCES, ransac_msac_command(), force, verbose)


def build_ransac_lo(force=False, verbose=False):
    return _build_one(RANSAC_LO_OUT, RANSAC_LO_RESOURCES, RANSAC_LO_SOURCES, ransac_lo_command(), force, verbose)


def build_ransac_pnpl_lo(force=False, verbose=False):
    return _build_one(RANSAC_PNPL_LO_OUT, RANSAC_PNPL_LO_RESOURCES, RANSAC_PNPL_LO_SOURCES, ransac_pnpl_lo_command(), force, verbose)


def build(force=False, verbose=False):
    """All fifteen libraries; returns the solver's (OUT)."""
    _build_one(OUT, RESOURCES, DEPS, compile_cmd(), force, verbose)
    build_grad(force, verbose)
    build_ransac(force, verbose)
    build_ransac_pnpl(force, verbose)
    build_refine(force, verbose)
    build_refine_grad(force, verbose)
    build_refine_robust(force, verbose)
    build_refine_robust_grad(force, verbose)
    build_ransac_adaptive(force, verbose)
    build_ransac_guided(force, verbose)
    build_ransac_pnpl_adaptive(force, verbose)
    build_refine_robust_auto(force, verbose)
    build_ransac_msac(force, verbose)
    build_ransac_lo(force, verbose)
    build_ransac_pnpl_lo(force, verbose)
    return OUT


def kernel_resources(path=RESOURCES):
    """{demangled kernel name: {"vgpr", "agpr", "scratch", "occupancy", "sgpr_spill", "vgpr_spill", "lds"}} from the remarks of a build"""
    import re

    rows, cur = [], None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    names = subprocess.run(["c++filt"] + [r["name"] for r in rows], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for r, d in zip(rows, names):
        d = re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")).replace("void ", "")
        out[d] = {"vgpr": int(r.get("VGPRs", -1)), "agpr": int(r.get("AGPRs", -1)), "scratch": int(r.get("ScratchSize [bytes/lane]", -1)),
                  "occupancy": int(r.get("Occupancy [waves/SIMD]", -1)), "sgpr_spill": int(r.get("SGPRs Spill", -1)),
                  "vgpr_spill": int(r.get("VGPRs Spill", -1)), "lds": int(r.get("LDS Size [bytes/block]", -1))}
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
