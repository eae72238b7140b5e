"""-m gpu: the solve options steplimit, ls_mu, ls_eta, ls_maxfev and opttol at NON-DEFAULT values, on every kernel that consumes them
(sqp_wave_kernel in its register form and in its LDS-state form, sqp_kernel with and without the augmented-Lagrangian loop), against the
oracle run under the same options.  The cases are tests/solve_option_cases.py; tests/test_solve_option_cases.py shows on the CPU that each
is sensitive to its option and insensitive to rounding, which is why inform, iters and nfev are asserted EQUAL per problem here.
Objective and x to the tolerances of test_gpu_solve.py's fixed-work parity tests: 1e-7 relative, 1e-5 max|x_ref|."""
import numpy as np
import pytest
import torch

import orc
import solve_option_cases as soc
from ntg_amd import api
from gpu_common import dev, rel
from wave_golden_cases import scaled_grids

pytestmark = pytest.mark.gpu

_plans = {}
VALUE_KEYS = ("x", "objective", "nfev", "iters", "inform")


def plan_of(case):
    name = soc.CASES[case][0]
    if name not in _plans:
        _plans[name] = api.Plan(soc.PLANS[name][0](), 0)
    return _plans[name]


def gpu_solve(plan, lo, up, x0, kw, want_lambda=False):
    x = dev(x0)
    out = plan.solve(dev(lo), dev(up), x, api.default_opts(**kw), want_lambda=want_lambda)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["x"] = x.cpu().numpy()
    return res


def assert_counts_equal(out, ref):
    for k in ("inform", "iters", "nfev"):
        assert np.array_equal(out[k], ref[k]), (k, out[k], ref[k])


@pytest.mark.parametrize("case", list(soc.CASES))
def test_option_case_matches_oracle(case):
    spec, lo, up, x0, kw, kernel, kind = soc.problem(case)
    plan = plan_of(case)
    nb = lo.shape[0]
    assert plan.solve_kernel(nb, api.default_opts(**kw)) == kernel
    out = gpu_solve(plan, lo, up, x0, kw)
    ref = orc.solve_batch(spec, lo, up, x0, orc.default_opts(**kw), nthreads=8)
    print(case, "gpu nfev/iters/inform", out["nfev"], out["iters"], out["inform"], "| oracle", ref["nfev"], ref["iters"], ref["inform"],
          "| rel dF", rel(out["objective"], ref["objective"]), "dx", np.abs(out["x"] - ref["x"]).max() / np.abs(ref["x"]).max())
    assert_counts_equal(out, ref)
    assert rel(out["objective"], ref["objective"]) <= 1e-7
    assert np.abs(out["x"] - ref["x"]).max() <= 1e-5 * np.abs(ref["x"]).max()
    if kind == "fail":
        assert (out["inform"] == 6).all() and (out["iters"] == 0).all() and (out["nfev"] == soc.fail_nfev(kw)).all()


ZEROED = dict(steplimit=0.0, ls_mu=0.0, ls_eta=0.0, ls_maxfev=0, opttol=0.0)
NEGATIVE = dict(steplimit=-0.3, ls_mu=-0.6, ls_eta=-0.1, ls_maxfev=-3, opttol=-1e-2)


@pytest.mark.parametrize("case,base", [("M_steplimit0.3", dict(itlim=12, fixed_iters=1)), ("M_opttol1e-2", dict(hessian=1)),
                                       ("A_eta0.1", dict(itlim=6, fixed_iters=1)), ("A_opttol1e-3", dict())],
                         ids=["M_fixed12", "M_precond", "A_fixed6", "A_to_convergence"])
def test_zero_and_negative_values_mean_the_defaults(case, base):
    """a value <= 0 of any of the five options selects its default: bit-identical to the solve that names the defaults.  (The negative
    values are, sign apart, values that change the result of these very problems: taken by magnitude they would show.)"""
    spec, lo, up, x0, _, kernel, _ = soc.problem(case)
    plan = plan_of(case)
    d = api.default_opts()
    assert (d.steplimit, d.ls_mu, d.ls_eta, d.ls_maxfev, d.opttol) == (2.0, 1e-4, 0.9, 20, 0.0)
    assert plan.solve_kernel(lo.shape[0], api.default_opts(**base)) == kernel
    want = gpu_solve(plan, lo, up, x0, base)
    for other in (ZEROED, NEGATIVE):
        got = gpu_solve(plan, lo, up, x0, dict(base, **other))
        for k in VALUE_KEYS:
            assert np.array_equal(got[k], want[k]), (k, other)


@pytest.mark.parametrize("case", ["M_steplimit0.3", "M_mu0.6_maxfev3"])
def test_options_reach_the_grids_instance_and_the_multiplier_pass(case):
    """the per-problem-grids instance of the wave kernel and the pass for the multipliers take the options from the same argument
    segment: the same counts as the plain solve of the case (the grids change the problems' scaling, not the branch the search takes).
    On the failure exit the multipliers are those at the projected start: finite, none on the coefficients' own bounds"""
    spec, lo, up, x0, kw, kernel, kind = soc.problem(case)
    nb = lo.shape[0]
    plain = gpu_solve(plan_of(case), lo, up, x0, kw)
    lam = gpu_solve(plan_of(case), lo, up, x0, kw, want_lambda=True)
    assert_counts_equal(lam, plain)
    assert np.array_equal(lam["x"], plain["x"]) and np.array_equal(lam["objective"], plain["objective"])
    assert np.isfinite(lam["clambda"]).all() and (lam["clambda"][:, :spec.nC] == 0).all()
    if kind != "fail":
        assert np.abs(lam["clambda"][:, spec.nC:]).max() > 0
    gplan = api.Plan(spec, 0)
    kn, bpg = scaled_grids(spec, nb)
    gplan.set_grids(dev(kn), dev(bpg), with_precond=False)
    assert gplan.solve_kernel(nb, api.default_opts(**kw)) == kernel
    grids = gpu_solve(gplan, lo, up, x0, kw)
    assert_counts_equal(grids, plain)
    assert np.isfinite(grids["x"]).all() and np.isfinite(grids["objective"]).all()
    assert not np.array_equal(grids["objective"], plain["objective"])           # other grids: other problems
