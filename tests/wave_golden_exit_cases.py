"""The cases of tests/test_gpu_wave_golden_exits.py, shared with tools/record_wave_golden.py --exits (which records the fixture
tests/golden/wave_exits.npz): solves of sqp_wave_kernel that END AT THE ITERATION LIMIT -- the exit from the middle of the kernel's
nested loops, and the step whose quasi-Newton update nothing reads.  Each case solves the first 8 problems of
cf.kincar_random_bounds(ncars, 4096) from x = 1; config M with the identity cold start unless the case says otherwise.
  M_fixed_it1 / 2 / 3        the solve ends before a chain exists, or at one or two slots
  M_fixed_it17 / 21 / 31     the last step's sweep is the first into the second butterfly group (16 slots a group), into the LDS tier
                             (20 register slots) and into the HBM tier (30 slots on chip)
  M_mem24_fixed_it25 / 26    memory 24: the restart at the full memory and the head pair behind it fall on or next to the last step
  M_free_it5                 not fixed, identity cold start: the limit comes long before convergence, every problem ends inform 4
  M_precond_it2 / 3 / 4      hessian = 1, not fixed: the two-waves-per-SIMD instance.  All eight preconditioned solves meet the convergence
                             test at their third step.  Recorded: limit 2 -- all eight inform 4 after 2 majors; limit 3 -- all eight inform 0
                             after 3 majors (the convergence test and the limit meet at one step, and the convergence wins); limit 4 -- the
                             same 3 majors, the limit not reached.  No limit gives a mix of 0 and 4 inside one case on these eight problems
  M_fixed_it3_lambda         want_lambda: the pass for the multipliers behind the last step (clambda compared too)
  B_fixed_it3                config B: two outputs, three doubles per lane
  M_grids_fixed_it3          per-problem grids
  M_noagpr_fixed_it3         NTG_AMD_WAVE_NOAGPR: the instance without hand-managed registers"""
import os

import numpy as np
import torch

from ntg_amd import api, configs as cf
from wave_golden_cases import KEYS, NB, scaled_grids


def _fixed(itlim, **kw):
    return dict(itlim=itlim, fixed_iters=1, hessian=0, **kw)


# name -> (spec, cars, solve options, environment variable to set or None, per-problem grids, want_lambda)
CASES = {
    "M_fixed_it1": (cf.config_M, 3, _fixed(1), None, False, False),
    "M_fixed_it2": (cf.config_M, 3, _fixed(2), None, False, False),
    "M_fixed_it3": (cf.config_M, 3, _fixed(3), None, False, False),
    "M_fixed_it17": (cf.config_M, 3, _fixed(17), None, False, False),
    "M_fixed_it21": (cf.config_M, 3, _fixed(21), None, False, False),
    "M_fixed_it31": (cf.config_M, 3, _fixed(31), None, False, False),
    "M_mem24_fixed_it25": (cf.config_M, 3, _fixed(25, qn_memory=24), None, False, False),
    "M_mem24_fixed_it26": (cf.config_M, 3, _fixed(26, qn_memory=24), None, False, False),
    "M_free_it5": (cf.config_M, 3, dict(itlim=5, hessian=0), None, False, False),
    "M_precond_it2": (cf.config_M, 3, dict(itlim=2, hessian=1), None, False, False),
    "M_precond_it3": (cf.config_M, 3, dict(itlim=3, hessian=1), None, False, False),
    "M_precond_it4": (cf.config_M, 3, dict(itlim=4, hessian=1), None, False, False),
    "M_fixed_it3_lambda": (cf.config_M, 3, _fixed(3), None, False, True),
    "B_fixed_it3": (cf.config_B, 1, _fixed(3), None, False, False),
    "M_grids_fixed_it3": (cf.config_M, 3, _fixed(3), None, True, False),
    "M_noagpr_fixed_it3": (cf.config_M, 3, _fixed(3), "NTG_AMD_WAVE_NOAGPR", False, False),
}


def keys_of(name):
    return KEYS + (("clambda",) if CASES[name][5] else ())


def run_case(name):
    """solve the case on cuda:0 with the loaded library; {key: numpy array} for keys_of(name)"""
    mk, ncars, kw, env, grids, lam = CASES[name]
    spec = mk()
    lo, up = cf.kincar_random_bounds(ncars, 4096)
    lo, up = np.ascontiguousarray(lo[:NB]), np.ascontiguousarray(up[:NB])
    dev = torch.device("cuda:0")
    opts = api.default_opts(**kw)
    plan = api.Plan(spec, 0)
    before = os.environ.get(env) if env else None   # (read when the launch is planned: set around solve_kernel and solve only)
    if env:
        os.environ[env] = "1"
    try:
        if grids:
            kn, bpg = scaled_grids(spec, NB)
            plan.set_grids(torch.tensor(kn, device=dev), torch.tensor(bpg, device=dev), with_precond=False)
        kernel = plan.solve_kernel(NB, opts)
        assert kernel == "sqp_wave_kernel", kernel
        x = torch.ones((NB, spec.nC), dtype=torch.float64, device=dev)
        out = plan.solve(torch.tensor(lo, device=dev), torch.tensor(up, device=dev), x, opts, want_lambda=lam)
        torch.cuda.synchronize()
    finally:
        if env and before is None:
            os.environ.pop(env, None)
        elif env:
            os.environ[env] = before
    res = {k: out[k].cpu().numpy() for k in keys_of(name) if k != "x"}
    res["x"] = x.cpu().numpy()
    return res
