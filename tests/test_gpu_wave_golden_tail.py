"""-m gpu: the chain's tail in HBM reproduces recorded results bit for bit on the one-wave-per-SIMD instances, whatever layout the tier
has in the launch's workspace.  The fixture tests/golden/wave_tail.npz was recorded with tools/record_wave_golden.py --tail from the
library of the commit before the tier's slots moved to 16-byte requests; the cases (short tails, a chain of more than 64 slots, an odd
number of doubles per lane) are in tests/wave_golden_tail_cases.py.  Coefficients, objective, inform, iterations and evaluation counts
are compared, the floats by their bit patterns."""
import os

import numpy as np
import pytest

import wave_golden_tail_cases as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_tail.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(wc.CASES))
def test_tail_bitwise(golden, name):
    got = wc.run_case(name)   # (asserts that the solve runs on sqp_wave_kernel)
    if wc.CASES[name][3] is not None:
        assert (got["iters"] == wc.CASES[name][3]).all()
    else:
        assert (got["iters"] > 72).all()   # past the restart at the chain's capacity (74 slots)
    for k in ("iters", "nfev", "inform"):
        assert np.array_equal(got[k], golden[name + "/" + k]), k
    # bitwise: compare the bit patterns (array_equal on floats would also accept -0.0 == 0.0)
    for k in ("objective", "x"):
        assert np.array_equal(got[k].view(np.int64), golden[name + "/" + k].view(np.int64)), k
