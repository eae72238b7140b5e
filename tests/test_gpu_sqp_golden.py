"""-m gpu: the structured Newton mode and the QP-based SQP step of sqp_kernel reproduce recorded results bit for bit.  The fixture
tests/golden/sqp_modes.npz was recorded with tools/record_wave_golden.py --sqp from the library of the commit before the wave's passive-set
solve became a function of qpdual.hpp and the host took the modes' memory from nwt_map.hpp: what any later restructuring of the two modes has to
reproduce.  The cases (every layout and entry of the two modes at its smallest shape) are in tests/sqp_golden_cases.py.  Coefficients, objective, multipliers, inform,
iterations, evaluation counts and the modes' work counters are compared, the floats by their bit patterns; the kernel the plan names for
the solve is the recorded one."""
import os

import numpy as np
import pytest

import sqp_golden_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sqp_modes.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_every_recorded_solve_ended_optimal(golden):
    for name in sc.CASES:
        assert np.isin(golden[name + "/inform"], (0, 1)).all(), name


@pytest.mark.parametrize("name", list(sc.CASES))
def test_modes_bitwise(golden, name):
    got, kernel = sc.run_case(name)
    assert kernel == str(golden[name + "/kernel"])
    assert kernel == ("sqp_kernel" if name != "B_h2" else "sqp_wave_kernel")
    for k in ("iters", "nfev", "inform"):
        assert np.array_equal(got[k], golden[name + "/" + k]), k
    # bitwise: compare the bit patterns (array_equal on floats would also accept -0.0 == 0.0)
    for k in ("objective", "x", "clambda", "counters"):
        assert np.array_equal(got[k].view(np.int64), golden[name + "/" + k].view(np.int64)), k
