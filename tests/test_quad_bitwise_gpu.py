"""The quad-schedule kernels (cvxq::solve_quad_kernel, csrc/quad_kernel.h) against outputs recorded from the parent of the change that
re-ordered the LDS reads of the iteration's short phases (G = (W + sigma I) V, W+, projection + update; profiles/r08/quad_lds_phases_ab.txt).

That change moves loads and interleaves independent chains; every value is computed by the same operations in the same order.  So every
array of tests/golden/quad_parent_outputs.npz -- recorded on an MI355X from a build of the parent commit's sources by
tests/golden/make_golden_quad_parent.py, which also holds the list of cases -- must equal what the library under test returns, element for
element; float arrays are compared as bytes (NaN equals NaN, -0 differs from +0).  A last-bit difference means an operation was reordered
or contracted differently: pin the operation sequence in the kernel with explicit fma / products, do not loosen this test.

The cases are the smallest shapes at which the edited code can go wrong: a partial last wavefront whose surplus rows redo the last problem
(batches 257, 259, 131, 61, 67), rows that finish at different iterations, columns without a positive eigenvalue, and every instantiation
that shares the edited helpers (both sweep precisions, lines, the rc variant, the two MODE 2 kernels of minimal problems, the twelve-lane
penta layout, the cost seam).

THE FIXTURE MUST BE REGENERATED FROM THE PARENT of any later change that alters the arithmetic of these kernels on purpose (run the
generator on that parent's build, commit the new file with the change, and say so in the change).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_quad_parent", os.path.join(HERE, "golden", "make_golden_quad_parent.py"))
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
    with np.load(os.path.join(HERE, "golden", "quad_parent_outputs.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(recorded):
    want = set()
    for name in gen.CASES:
        want |= set(gen.stored(name, {k: np.zeros(1) for k in gen.INTS + gen.FLOATS}))
    assert set(recorded) == want


@pytest.mark.parametrize("name", list(gen.CASES))
def test_outputs_equal_the_parents_bit_for_bit(gpu, recorded, name):
    out = gen.run_case(name, gpu)
    batch = gen.CASES[name][2]
    assert out["status"].shape == (batch,) and out["R"].shape == (batch, 3, 3)
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
