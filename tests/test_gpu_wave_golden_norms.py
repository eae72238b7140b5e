"""-m gpu: solves through the consumers of the iterate's norms and of |g|^2 reproduce recorded results bit for bit.  On the
one-wave-per-SIMD instances of sqp_wave_kernel (solve_wave.hpp) the square roots of the totals that come out of the 16-wide butterflies
(|d| at the first major, |x|, |gp|, |s|, |y|) are taken in lanes before the broadcast, and |g|^2 -- read by the tolerance tolg alone --
is no longer summed over the wave at every evaluation: the evaluation site sums two values, and |g|^2 of an accepted point rides with
the two products of the new direction.  The fixed-work solve of the other golden files passes through none of the places that read
tolg, and through the norms only where every trial takes the full step; the cases here (tests/wave_golden_norms_cases.py) are the solves
that do: convergence at three tolerances, line searches cut to 1, 2 and 3 evaluations, step limits that make |x| / |d| the first trial,
a tolerance nothing meets (line-search failures with and without a restart), the iteration limit next to ST_INIT, and the other
one-wave instances to convergence.  The fixture tests/golden/wave_norms.npz was recorded with tools/record_wave_golden.py --norms from
the library of the commit before the change.  Coefficients, objective, inform, iterations and evaluation counts are compared, the
floats by their bit patterns.  The branch pnorm == 0 at a major's start has no known trigger: it is covered by reading only."""
import os

import numpy as np
import pytest

import wave_golden_norms_cases as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_norms.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_left_the_main_path(golden):
    """what the recorded results must contain for the cases to test what they say (no solve): exits by convergence (0), by a failed
    line search (1 or 6) and at the iteration limit (4)"""
    informs = np.concatenate([golden[n + "/inform"] for n in wc.CASES])
    assert (informs == 0).any() and ((informs == 1) | (informs == 6)).any() and (informs == 4).any(), np.unique(informs)
    for name, (_, _, kw, *_rest) in wc.CASES.items():
        assert golden[name + "/inform"].shape == (_rest[-1],), name
        if kw.get("fixed_iters") and kw.get("ls_maxfev") != 1:
            assert (golden[name + "/iters"] == kw["itlim"]).all() and (golden[name + "/inform"] == 4).all(), name
    # the loosened tolerances end the solves at earlier majors; the unreachable one ends none by convergence
    assert golden["M_conv_tol1e6/iters"].sum() < golden["M_conv_tol1e3/iters"].sum() < golden["M_conv/iters"].sum()
    assert (golden["M_tol1e-30_it300/inform"] != 0).all()
    # a step limit below the full step: one evaluation per major where 0.05 (1 + |x|) / |d| is accepted at once
    assert (golden["M_step0.05_fixed10/nfev"] < golden["M_step0.5_fixed10/nfev"]).all()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_norms_bitwise(golden, name):
    got = wc.run_case(name)   # (asserts that the solve runs on sqp_wave_kernel)
    for k in ("iters", "nfev", "inform"):
        assert np.array_equal(got[k], golden[name + "/" + k]), k
    # bitwise: compare the bit patterns (array_equal on floats would also accept -0.0 == 0.0)
    for k in ("x", "objective"):
        assert np.array_equal(got[k].view(np.int64), golden[name + "/" + k].view(np.int64)), k
