"""The cases of tests/test_solve_option_cases.py (CPU: why each case is admitted) and tests/test_gpu_solve_options.py (GPU: parity with
the oracle): solves under NON-DEFAULT values of the solve options steplimit, ls_mu, ls_eta, ls_maxfev and opttol.  Every case is a batch
solved from x = 1; the expectation is the oracle's own run under the same options, never a recorded figure.

Why these inputs.  The kincar cost is quadratic: with default options the first trial a = 1 fails Armijo, the cubic step lands on the exact
minimiser and the second trial is accepted -- two evaluations per line search whatever ls_eta, ls_mu (< 0.5) and ls_maxfev (>= 2) say.
The options show on that cost only where they change which branch the search takes:
  steplimit      caps the first trial below 1: it passes Armijo at once, one evaluation per major, and the iterates are others
  ls_mu = 0.6    the exact minimiser of a quadratic gives a decrease of 0.5 a phi'(0): Armijo with mu > 0.5 can never hold, the search spends
                 its whole budget and fails (inform 6 at major 0, x = the projected start, nfev = 1 + ls_maxfev)
  ls_maxfev = 1  the budget is spent at the first, rejected, trial: the same failure after 2 evaluations
  ls_eta = 1e-30, ls_maxfev = 3
                 no trial meets the curvature test; the third evaluation spends the budget inside the zoom and the search evaluates at
                 a_lo and accepts unconditionally (LineSearch::step returning 2): 4 evaluations per major
  opttol         the convergence test fires at another major
Config A (vanderpol: a non-quadratic cost on sqp_kernel) and O8 (the obstacle row: sqp_kernel's augmented-Lagrangian loop) respond to every
one of the options in their counts.

Left out because rounding decides them (the oracle's counts move under a 1e-13 perturbation of the start): ls_eta = 1e-30 with
ls_maxfev = 4 or with hessian = 1, config M with hessian = 1 under ls_eta close to 1, K0 with steplimit = 0.3.  On the O plan the oracle
answers inform 9 to fixed_iters = 1, so those cases carry itlim alone."""
import numpy as np

from ntg_amd import configs as cf

NB = 8
WAVE, WG = "sqp_wave_kernel", "sqp_kernel"


def _kincar(ncars):
    return lambda: cf.kincar_random_bounds(ncars, NB)


def _bounds_A():
    b = np.tile(cf.bounds_A()[0], (NB, 1)) + np.random.default_rng(3).uniform(-0.3, 0.3, (NB, 3))
    return b.copy(), b.copy()


def _bounds_K0():
    lo, up = cf.bounds_K0_shipped()
    return lo[None].copy(), up[None].copy()


def _o8():
    return cf.config_O(ninterv=8)


# plan name -> (spec, bounds [batch, nbounds] lower and upper, the kernel its solves must run on)
PLANS = {
    "M": (cf.config_M, _kincar(3), WAVE),
    "B": (cf.config_B, _kincar(1), WAVE),
    "K0": (cf.config_K0, _bounds_K0, WG),          # order 5 on 2 intervals: outside the wave kernel's class; a batch of one
    "A": (cf.config_A, _bounds_A, WG),
    "O8": (_o8, lambda: cf.obstacle_bounds(NB), WG),
}

_FIX12 = dict(itlim=12, fixed_iters=1)
_FIX6 = dict(itlim=6, fixed_iters=1)
_O8 = dict(hessian=1, itlim=6)

# name -> (plan, solve options besides the defaults, kind)
#   kind "ok":       compared with the oracle
#   kind "fail":     the line search fails at the first major: additionally inform 6, iters 0, nfev = fail_nfev(options)
#   kind "baseline": the default options on a plan whose other cases are read against it (it cannot differ from itself)
CASES = {}


def _add(name, plan, opts, kind="ok"):
    assert name not in CASES
    CASES[name] = (plan, dict(opts), kind)


for _p in ("M", "B"):
    _add(f"{_p}_steplimit0.3", _p, dict(_FIX12, steplimit=0.3))
    for _m in (2, 3, 5, 20):
        _add(f"{_p}_mu0.6_maxfev{_m}", _p, dict(_FIX12, ls_mu=0.6, ls_maxfev=_m), "fail")
    _add(f"{_p}_maxfev1", _p, dict(_FIX12, ls_maxfev=1), "fail")
_add("M_steplimit0.01", "M", dict(itlim=3, fixed_iters=1, steplimit=0.01))
_add("M_precond_steplimit0.3", "M", dict(hessian=1, itlim=4, fixed_iters=1, steplimit=0.3))       # the two-waves-per-SIMD (LDS-state) instance
_add("M_precond_mu0.6_maxfev3", "M", dict(hessian=1, ls_mu=0.6, ls_maxfev=3), "fail")               # the same instance
_add("K0_mu0.6_maxfev5", "K0", dict(itlim=6, fixed_iters=1, ls_mu=0.6, ls_maxfev=5), "fail")
_add("M_forced_accept", "M", dict(_FIX6, ls_eta=1e-30, ls_maxfev=3))
_add("M_opttol1e-2", "M", dict(opttol=1e-2, itlim=400))
_add("M_opttol1e-3", "M", dict(opttol=1e-3, itlim=400))
_add("M_precond_opttol1e-3", "M", dict(hessian=1, opttol=1e-3))
_add("A_eta0.1", "A", dict(_FIX6, ls_eta=0.1))
_add("A_eta0.01", "A", dict(_FIX6, ls_eta=0.01))
_add("A_maxfev2", "A", dict(_FIX6, ls_maxfev=2))
_add("A_maxfev3_eta0.1", "A", dict(_FIX6, ls_maxfev=3, ls_eta=0.1))
_add("A_steplimit0.05", "A", dict(_FIX6, steplimit=0.05))
_add("A_mu0.3_eta0.35", "A", dict(_FIX6, ls_mu=0.3, ls_eta=0.35))
_add("A_opttol1e-3", "A", dict(opttol=1e-3))
_add("A_opttol1e-5", "A", dict(opttol=1e-5))
_add("A_opttol1e-3_eta0.1", "A", dict(opttol=1e-3, ls_eta=0.1))
_add("O8_default", "O8", _O8, "baseline")
_add("O8_eta0.1", "O8", dict(_O8, ls_eta=0.1))
_add("O8_maxfev3", "O8", dict(_O8, ls_maxfev=3))
_add("O8_steplimit0.1", "O8", dict(_O8, steplimit=0.1))

# The drop-in path (ntg() of include/ntg.h, options as strings through npsoloption()): tests/test_gpu_dropin.py.
# name -> (problem of tests/drivers/dropin_drv.c, option string under test, the oracle's options for it, companion string or None, the
# oracle's options for the companion).  Both shipped problems are solved to the same optimum whatever the line search and the step limit do
# on the way, and kincar meets every tolerance at its second major: run to convergence, most of the strings leave inform and objective
# where they were, and an ignored string would pass.  Such a string is therefore also run next to a companion option that stops the
# solve where the string's effect still shows (an iteration limit), or that gives it something to act on (a step limit that makes kincar
# take many majors); the run with both is read against the run with the companion alone.
DROPIN_PROBLEMS = {"vanderpol": (cf.config_A, cf.bounds_A), "kincar": (cf.config_K0, cf.bounds_K0_shipped)}
_ETA, _STEP, _ITLIM, _OPTTOL = "line search tolerance = 0.1", "step limit 0.05", "major iteration limit = 6", "optimality tolerance = 1e-3"
DROPIN = {
    "vanderpol_eta": ("vanderpol", _ETA, dict(ls_eta=0.1), "major iteration limit = 5", dict(itlim=5)),
    "vanderpol_steplimit": ("vanderpol", _STEP, dict(steplimit=0.05), "major iteration limit = 6", dict(itlim=6)),
    "vanderpol_itlim": ("vanderpol", _ITLIM, dict(itlim=6), None, {}),
    "vanderpol_opttol": ("vanderpol", _OPTTOL, dict(opttol=1e-3), None, {}),
    "kincar_eta": ("kincar", _ETA, dict(ls_eta=0.1), "major iteration limit = 1", dict(itlim=1)),
    "kincar_steplimit": ("kincar", _STEP, dict(steplimit=0.05), "major iteration limit = 3", dict(itlim=3)),
    "kincar_itlim": ("kincar", _ITLIM, dict(itlim=6), "step limit 0.03", dict(steplimit=0.03)),
    "kincar_opttol": ("kincar", _OPTTOL, dict(opttol=1e-3), "step limit 0.005", dict(steplimit=0.005)),
}


def differs(a, b):
    """what tells two solves of one problem apart at the drop-in boundary: inform, or the objective by more than 1e-6 relative"""
    return a["inform"] != b["inform"] or abs(a["objective"] - b["objective"]) > 1e-6 * abs(b["objective"])


# the options under test; a case's remaining options (itlim, fixed_iters, hessian) are the ones its default-options twin keeps
VARIED = ("steplimit", "ls_mu", "ls_eta", "ls_maxfev", "opttol")


def problem(name):
    """(spec, lower, upper, x0, solve options, kernel expected, kind) of a case"""
    plan, opts, kind = CASES[name]
    mk, bounds, kernel = PLANS[plan]
    spec = mk()
    lo, up = bounds()
    lo, up = np.ascontiguousarray(lo), np.ascontiguousarray(up)
    return spec, lo, up, np.ones((lo.shape[0], spec.nC)), dict(opts), kernel, kind


def default_twin(opts):
    """the case's options with every option under test back at its default"""
    return {k: v for k, v in opts.items() if k not in VARIED}


def fail_nfev(opts):
    """evaluations of a solve whose first line search fails: F at the projected start, then the search's whole budget (no trial passed
    Armijo, so there is no best step to fall back to and nothing more is evaluated)"""
    return 1 + opts.get("ls_maxfev", 20)
