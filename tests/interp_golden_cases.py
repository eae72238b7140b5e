"""The cases of tests/test_gpu_interp_golden.py, shared with tools/record_cert_golden.py (set `interp`, which records the fixture
tests/golden/interp_calls.npz): Plan.interp on inputs small enough to store, so that a change of the host side of ntg_batch_interp_strided
(who builds the basis at the times, in which scratch, in how many chunks) can be held to the recorded flags bit for bit.  The fixture
stores the inputs next to z; the test replays the stored inputs.

  T     the shared grid with two basis classes: config T of tests/test_gpu_basis_eval.py::test_batch_interp_matches_spline_interp, whose
        last output has another order and another number of knot intervals than the rest.  Batch 5, 9 times: both ends of the horizon,
        an interior knot of either class with the doubles next to it on both sides, one time between knots.
  PP    per-problem grids: the plan and grids of tests/test_gpu_grids.py::test_interp_on_per_problem_grids (config M, warped knots) with
        batch 5 and 7 times per problem, times [batch][ntimes]: both ends of the problem's own horizon, its knot 2 with the doubles next
        to it on both sides, two times between knots.
  PP0   the same plan and x with one time vector for the batch (times_stride = 0): the common start, the end of the shortest horizon,
        knot 2 of problem 1 with its two neighbours, two times between.
These are the places where interv_breaks and the offsets can go wrong."""
import numpy as np

from gpu_common import dev
from ntg_amd import api, configs as cf

CASES = ["T", "PP", "PP0"]
NB = 5


def _around(t):
    return [np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)]


def inputs(name):
    """{name: numpy array}: x [NB, nC], times, and for per-problem grids knots and bps"""
    if name == "T":
        spec = cf.config_T()
        rng = np.random.default_rng(31)
        t0, t1 = float(spec.bps[0]), float(spec.bps[-1])
        times = np.array([t0, t1] + _around(float(spec.knots[0][2])) + _around(float(spec.knots[-1][3])) + [rng.uniform(t0, t1)])
        assert len(set(spec.kninterv)) == 2 and len(times) == 9
        return dict(x=rng.normal(size=(NB, spec.nC)), times=times)
    from test_gpu_grids import grids_for
    spec = cf.config_M()
    knots, bps = grids_for(spec, NB, warp=0.3, seed=3)
    rng = np.random.default_rng(8)
    x = rng.normal(size=(NB, spec.nC))
    if name == "PP":
        times = np.stack([np.array([knots[b, 0], knots[b, -1]] + _around(knots[b, 2]) + list(rng.uniform(knots[b, 0], knots[b, -1], 2))) for b in range(NB)])
    else:
        end = knots[:, -1].min()
        times = np.array([knots[:, 0].max(), end] + _around(knots[1, 2]) + list(rng.uniform(knots[:, 0].max(), end, 2)))
        assert knots[1, 2] < end
    assert times.shape[-1] == 7
    return dict(x=x, times=times, knots=knots, bps=bps)


def plan_of(name, inp):
    """the case's plan, per-problem grids set"""
    plan = api.Plan(cf.config_T() if name == "T" else cf.config_M(), 0)
    if name != "T":
        plan.set_grids(dev(inp["knots"]), dev(inp["bps"]), with_precond=False)
    return plan


def run(name, inp):
    """z [NB, ntimes, nz] of the case's plan on the stored inputs, on cuda:0 with the loaded library"""
    return plan_of(name, inp).interp(dev(inp["x"]), dev(inp["times"])).cpu().numpy()


def run_case(name):
    inp = inputs(name)
    return dict(inp, z=run(name, inp))
