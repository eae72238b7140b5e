"""-m gpu: the instances of sqp_wave_kernel that share the chain sweep with the headline one reproduce recorded results bit for bit
(tests/test_gpu_wave_golden.py pins the headline instance only).  The fixture tests/golden/wave_instances.npz was recorded with
tools/record_wave_golden.py from the library of the commit before the sweep's loads were pipelined; the cases are in
tests/wave_golden_cases.py.  Scheduling and register work on the sweep must not move a bit in any of them: coefficients, objective,
inform, iterations and evaluation counts are compared."""
import os

import numpy as np
import pytest

import wave_golden_cases as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_instances.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(wc.CASES))
def test_instance_bitwise(golden, name):
    got = wc.run_case(name)   # (asserts that the solve runs on sqp_wave_kernel)
    if name.endswith("fixed50"):
        assert (got["iters"] == 50).all()
    for k in ("iters", "nfev", "inform"):
        assert np.array_equal(got[k], golden[name + "/" + k]), k
    # bitwise: compare the bit patterns (array_equal on floats would also accept -0.0 == 0.0)
    for k in ("objective", "x"):
        assert np.array_equal(got[k].view(np.int64), golden[name + "/" + k].view(np.int64)), k


def test_no_register_slot_case_is_another_instance(golden):
    """Nothing reports which instance a solve ran on.  The case with NTG_AMD_WAVE_NOAGPR set must reproduce its fixture bitwise (above),
    and that fixture differs from the headline instance's results for the same problems -- the tiers add the chain's terms in another
    order -- so a run that ignored the variable would not pass."""
    head = np.load(os.path.join(os.path.dirname(GOLDEN), "wave_m_fixed50_64.npz"))
    a, b = golden["M_noagpr_fixed50/x"], head["x"][:wc.NB]
    assert a.shape == b.shape and not np.array_equal(a.view(np.int64), b.view(np.int64))
