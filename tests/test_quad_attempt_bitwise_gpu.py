"""The certificate attempt of the quad-schedule kernels (cvxq::solve_quad_kernel, csrc/quad_kernel.h: Newton polish, dual fit, quad_ldl, outputs)
against outputs recorded from the parent of the change that keeps the attempt's LDS reads in flight (profiles/r09/quad_attempt_lds_ab.txt).

That change issues loads earlier and replaces EXEC-masked arms by selects; every value is computed by the same operations in the same order.
So every array of tests/golden/quad_attempt_parent_outputs.npz -- recorded on an MI355X from a build of the parent commit's sources by
tests/golden/make_golden_quad_attempt_parent.py, which also holds the list of cases -- must equal what the library under test returns,
element for element: status, iters, work, R, t, cost and the SDP solution Z, the float arrays compared as bytes (NaN equals NaN, -0 differs
from +0).  A last-bit difference means an operation was reordered or contracted differently: pin the operation sequence in the kernel with
explicit fma / products, do not loosen this test.

tests/test_quad_bitwise_gpu.py covers every instantiation, but its problems are nearly all certified at their first attempt.  The cases
here are the ones in which attempts FAIL, so that the LDL^T meets negative, zero and NaN pivots (it does not stop on them) and rows of one
wavefront leave at different attempts: six noisy points (the full relaxation and the rc variant, batches 61 and 67: a partial last
wavefront), four points (the MODE 2 kernel <2,2,16,true,0>), and the cost seam with indefinite costs and one NaN.

THE FIXTURE MUST BE REGENERATED FROM THE PARENT of any later change that alters the arithmetic of these kernels on purpose (run the
generator on that parent's build, commit the new file with the change, and say so in the change).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_quad_attempt_parent", os.path.join(HERE, "golden", "make_golden_quad_attempt_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from cvxpnpl_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "quad_attempt_parent_outputs.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(recorded):
    assert set(recorded) == gen.keys()


def test_recorded_cases_are_the_hard_ones(recorded):
    """the conditions the cases were chosen by, on the parent's arrays"""
    for name in gen.CASES:
        if gen.noisy(name):
            assert float(recorded[f"{name}__sigma"]) in gen.NOISE_LEVELS
            assert (recorded[f"{name}__iters"] > gen.CASES[name][5]).mean() >= gen.NOISY_SHARE, name
        if gen.CASES[name][0] == "cost":
            assert (recorded[f"{name}__status"] != gen.ST_CERTIFIED).any(), name


@pytest.mark.parametrize("name", list(gen.CASES))
def test_outputs_equal_the_parents_bit_for_bit(gpu, recorded, name):
    out = gen.run_case(name, gpu, recorded[f"{name}__sigma"] if gen.noisy(name) else None)
    batch = gen.CASES[name][2]
    assert out["status"].shape == (batch,) and out["R"].shape == (batch, 3, 3) and out["Z"].shape == (batch, 55)
    problems = []
    for key, got in gen.stored(name, out).items():
        ref = recorded[key]
        if got.dtype != ref.dtype or got.shape != ref.shape:
            problems.append(f"{key}: {got.dtype} {got.shape}, recorded {ref.dtype} {ref.shape}")
        elif got.tobytes() != ref.tobytes():
            if key.endswith(".sha256"):
                problems.append(f"{key}: digest differs")
            else:
                bad = np.flatnonzero((got.reshape(batch, -1).view(np.uint8) != ref.reshape(batch, -1).view(np.uint8)).any(axis=1))
                problems.append(f"{key}: {bad.size} of {batch} problems differ, first {bad[:8].tolist()}")
    assert not problems, "\n".join(problems)
