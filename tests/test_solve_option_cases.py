"""CPU only: why each case of tests/solve_option_cases.py is admitted to the GPU parity test tests/test_gpu_solve_options.py.

(a) The option is visible: the oracle's result under the case's options differs from its result with the options under test at their
    defaults (same itlim, fixed_iters and hessian) -- in nfev, iters or inform of at least one problem, or in an objective by more than
    1e-6 relative.  A kernel that ignored the option would then fail the GPU comparison.
(b) The case is not decided by rounding: from six starts x0 (1 + 1e-13 N(0,1)) the oracle's nfev, iters and inform of EVERY problem are
    unchanged and the objective moves by at most 1e-9 relative.  The GPU kernels sum in other orders than the oracle; only a case whose
    branches survive a perturbation of that size can be asked for exactly equal counts.  No case is exempt: one that fails here is to
    be replaced by another input."""
import numpy as np
import pytest

import orc
import solve_option_cases as soc

NAMES = list(soc.CASES)
COUNTS = ("nfev", "iters", "inform")
_runs = {}


def oracle(name, opts, seed=None):
    """the oracle's solve of the case's problems under `opts`, from x = 1 or from the perturbed start of `seed`; computed once"""
    plan = soc.CASES[name][0]
    key = (plan, tuple(sorted(opts.items())), seed)
    if key not in _runs:
        spec, lo, up, x0, _, _, _ = soc.problem(name)
        if seed is not None:
            x0 = x0 * (1.0 + 1e-13 * np.random.default_rng(seed).standard_normal(x0.shape))
        _runs[key] = orc.solve_batch(spec, lo, up, x0, orc.default_opts(**opts), nthreads=8)
    return _runs[key]


def relobj(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize("name", NAMES)
def test_the_option_is_visible(name):
    opts, kind = soc.CASES[name][1], soc.CASES[name][2]
    if kind == "baseline":
        assert not set(opts) & set(soc.VARIED)     # the default run itself: the plan's other cases are read against it
        return
    assert set(opts) & set(soc.VARIED)
    r, d = oracle(name, opts), oracle(name, soc.default_twin(opts))
    differs = any(not np.array_equal(r[k], d[k]) for k in COUNTS) or bool((relobj(r["objective"], d["objective"]) > 1e-6).any())
    assert differs, {k: r[k] for k in COUNTS}


@pytest.mark.parametrize("name", NAMES)
def test_the_case_is_not_decided_by_rounding(name):
    opts = soc.CASES[name][1]
    r = oracle(name, opts)
    for seed in range(6):
        q = oracle(name, opts, seed)
        for k in COUNTS:
            assert np.array_equal(q[k], r[k]), (seed, k, q[k], r[k])
        assert relobj(q["objective"], r["objective"]).max() <= 1e-9, (seed, relobj(q["objective"], r["objective"]))


@pytest.mark.parametrize("name", [n for n in NAMES if soc.CASES[n][2] == "fail"])
def test_failed_search_spends_its_budget_and_returns_the_projected_start(name):
    """the inform-6 cases: every problem fails its first line search after the whole budget; x is the start projected onto the linear rows
    (feasible, and the same whatever the budget), the objective is F there"""
    spec, lo, up, x0, opts, _, _ = soc.problem(name)
    r = oracle(name, opts)
    assert (r["inform"] == 6).all() and (r["iters"] == 0).all() and (r["nfev"] == soc.fail_nfev(opts)).all()
    A = orc.export_tables(spec, lo[0], up[0])["A"]
    assert np.abs(r["x"] @ A.T - lo[:, :A.shape[0]]).max() <= 1e-8 * max(1.0, np.abs(lo).max())
    f = orc.eval_batch(spec, r["x"], 0)["f"]
    assert relobj(r["objective"], f).max() <= 1e-12


def dropin_oracle(problem, opts, seed=None):
    mk, bounds = soc.DROPIN_PROBLEMS[problem]
    spec = mk()
    lo, up = bounds()
    x0 = np.ones(spec.nC)
    if seed is not None:
        x0 = x0 * (1.0 + 1e-13 * np.random.default_rng(seed).standard_normal(spec.nC))
    return orc.solve_one(spec, lo, up, x0, orc.default_opts(**opts))


@pytest.mark.parametrize("name", list(soc.DROPIN))
def test_dropin_option_is_visible_and_not_decided_by_rounding(name):
    """the drop-in cases: next to its companion option the string under test changes inform or the objective (by the oracle), and neither
    run of the pair moves under a perturbed start -- counts unchanged, objective to 1e-9"""
    problem, _, kw, _, ckw = soc.DROPIN[name]
    assert not set(kw) & set(ckw)
    both, alone = dict(ckw, **kw), dict(ckw)
    assert soc.differs(dropin_oracle(problem, both), dropin_oracle(problem, alone))
    for opts in (both, alone):
        r = dropin_oracle(problem, opts)
        for seed in range(6):
            q = dropin_oracle(problem, opts, seed)
            assert (q["inform"], q["iters"], q["nfev"]) == (r["inform"], r["iters"], r["nfev"]), (opts, seed)
            assert abs(q["objective"] - r["objective"]) <= 1e-9 * abs(r["objective"])
