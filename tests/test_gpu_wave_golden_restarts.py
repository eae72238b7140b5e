"""-m gpu: the headline instance of sqp_wave_kernel with a quasi-Newton memory of 17 and of 21 reproduces recorded results bit for bit.
These memories restart the chain right behind a boundary of the groups of slots that pass 1 of the sweep reduces together (register
slots 0 .. 15, register slots 16 .. 19, the LDS tier; tests/wave_golden_restart_cases.py) -- chain lengths that the other golden tests
pass once on the way to 50 are the longest here, again and again.  The fixture tests/golden/wave_restarts.npz was recorded with
tools/record_wave_golden.py --restarts from the library of the commit before the DPP moves lost their zeroed operands: coefficients,
objective, inform, iterations and evaluation counts are compared as bit patterns."""
import os

import numpy as np
import pytest

import wave_golden_restart_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_restarts.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_restart_bitwise(golden, name):
    got = rc.run_case(name)   # (asserts that the solve runs on sqp_wave_kernel)
    assert (got["iters"] == 50).all()
    for k in ("iters", "nfev", "inform"):
        assert np.array_equal(got[k], golden[name + "/" + k]), k
    for k in ("objective", "x"):
        assert np.array_equal(got[k].view(np.int64), golden[name + "/" + k].view(np.int64)), k


def test_memories_differ(golden):
    """the two memories are different computations (a solve that ignored qn_memory would reproduce one fixture at the most)"""
    a, b = golden["M_memory17_fixed50/x"], golden["M_memory21_fixed50/x"]
    assert a.shape == b.shape and not np.array_equal(a.view(np.int64), b.view(np.int64))
