"""The cases of tests/test_gpu_wave_golden_norms.py, shared with tools/record_wave_golden.py --norms (which records the fixture
tests/golden/wave_norms.npz): solves of sqp_wave_kernel that pass through the CONSUMERS of the iterate's norms and of |g|^2 -- the
tolerance tolg = sr (1 + max(1 + |F|, |g|)) of the line search's failure branch, of the lost-definiteness branch and of the two
convergence tests; |x| / |d| in the first trial step; |gp| in the tests of a major's start.  On the one-wave-per-SIMD instances the
norms are rooted in lanes before the broadcast, and |g|^2 is summed over the wave at the first evaluation and at accepted steps only,
not at every evaluation, with tolg formed behind the tests that read it (solve_wave.hpp: NORMS, G2LATE); the fixed-work solve of the other golden files reads none of them.  Each case solves 8 or 16 problems of
cf.kincar_random_bounds(ncars, 4096) from x = 1 with the identity cold start (hessian = 0).
  M_conv / _tol1e3 / _tol1e6     config M to convergence at the default optimality tolerance and at 1e3 and 1e6 times it: the long-chain
                                 instance, the per-major test gpnorm <= 1e-3 tolg and the step test, exits at different majors
  M_fev1 / 2 / 3_fixed12, _conv  ls_maxfev = 1, 2, 3, with 12 fixed majors and to convergence: forced accepts and line-search failures
                                 (the rc != 1 branch reads tolg and gpnorm, with and without a restart from W0)
  M_step0.05 / 0.5_fixed10       steplimit: amax < 1, so |x| / |d| decides the first trial of every major
  M_tol1e-30_it300               a tolerance nothing meets (a case beyond the list above): every solve goes on until the line search
                                 fails at the noise level with updates in the chain -- the restart from W0 out of the rc != 1 branch,
                                 then the failure that ends the solve
  M_it0 / M_it1                  iteration limit 0 (the library's default limit: as M_conv, on the first 8 problems) and 1 (one major
                                 behind ST_INIT, then the limit)
  B_conv, M4b_conv, M_grids_conv, M_noagpr_conv
                                 the other one-wave-per-SIMD instances to convergence: two outputs, four outputs on 16 intervals,
                                 per-problem grids, no hand-managed registers
The option values were picked with the CPU oracle (tests/orc.py states the same iteration): over these cases it alone ends problems at
inform 0 (the solves to convergence), at 6 (ls_maxfev = 1: the first trial fails, no update to drop; the unreachable tolerance: failures
with and without a restart) and at 4 (the fixed-work cases, the limit of 1).  The branch pnorm == 0 of a major's start has no known trigger; it is covered by reading only."""
import os

import numpy as np
import torch

from ntg_amd import api, configs as cf
from wave_golden_cases import KEYS, _m4b, scaled_grids

OPTTOL0 = float(np.finfo(np.float64).eps) ** 0.8   # the default optimality tolerance (ntg_default_opts leaves 0: this value)


def _fixed(itlim, **kw):
    return dict(itlim=itlim, fixed_iters=1, hessian=0, **kw)


def _conv(**kw):
    return dict(hessian=0, **kw)


# name -> (spec, cars, solve options, environment variable to set or None, per-problem grids, first problem, problems)
CASES = {
    "M_conv": (cf.config_M, 3, _conv(), None, False, 8, 16),
    "M_conv_tol1e3": (cf.config_M, 3, _conv(opttol=1e3 * OPTTOL0), None, False, 8, 16),
    "M_conv_tol1e6": (cf.config_M, 3, _conv(opttol=1e6 * OPTTOL0), None, False, 8, 16),
    "M_fev1_fixed12": (cf.config_M, 3, _fixed(12, ls_maxfev=1), None, False, 0, 8),
    "M_fev2_fixed12": (cf.config_M, 3, _fixed(12, ls_maxfev=2), None, False, 0, 8),
    "M_fev3_fixed12": (cf.config_M, 3, _fixed(12, ls_maxfev=3), None, False, 0, 8),
    "M_fev1_conv": (cf.config_M, 3, _conv(ls_maxfev=1), None, False, 0, 8),
    "M_fev2_conv": (cf.config_M, 3, _conv(ls_maxfev=2), None, False, 0, 8),
    "M_fev3_conv": (cf.config_M, 3, _conv(ls_maxfev=3), None, False, 0, 8),
    "M_step0.05_fixed10": (cf.config_M, 3, _fixed(10, steplimit=0.05), None, False, 0, 8),
    "M_step0.5_fixed10": (cf.config_M, 3, _fixed(10, steplimit=0.5), None, False, 0, 8),
    "M_tol1e-30_it300": (cf.config_M, 3, _conv(opttol=1e-30, itlim=300), None, False, 0, 8),
    "M_it0": (cf.config_M, 3, _conv(itlim=0), None, False, 0, 8),
    "M_it1": (cf.config_M, 3, _conv(itlim=1), None, False, 0, 8),
    "B_conv": (cf.config_B, 1, _conv(), None, False, 0, 8),
    "M4b_conv": (_m4b, 2, _conv(), None, False, 0, 8),
    "M_grids_conv": (cf.config_M, 3, _conv(), None, True, 0, 8),
    "M_noagpr_conv": (cf.config_M, 3, _conv(), "NTG_AMD_WAVE_NOAGPR", False, 0, 8),
}


def bounds_of(name):
    """the case's bounds (lower, upper), each [problems, nbounds]"""
    _, ncars, _, _, _, first, nb = CASES[name]
    lo, up = cf.kincar_random_bounds(ncars, 4096)
    return np.ascontiguousarray(lo[first:first + nb]), np.ascontiguousarray(up[first:first + nb])


def run_case(name):
    """solve the case on cuda:0 with the loaded library; {key: numpy array} for KEYS"""
    mk, _, kw, env, grids, _, nb = CASES[name]
    spec = mk()
    lo, up = bounds_of(name)
    dev = torch.device("cuda:0")
    opts = api.default_opts(**kw)
    plan = api.Plan(spec, 0)
    before = os.environ.get(env) if env else None   # (read when the launch is planned: set around solve_kernel and solve only)
    if env:
        os.environ[env] = "1"
    try:
        if grids:
            kn, bpg = scaled_grids(spec, nb)
            plan.set_grids(torch.tensor(kn, device=dev), torch.tensor(bpg, device=dev), with_precond=False)
        kernel = plan.solve_kernel(nb, opts)
        assert kernel == "sqp_wave_kernel", kernel
        x = torch.ones((nb, spec.nC), dtype=torch.float64, device=dev)
        out = plan.solve(torch.tensor(lo, device=dev), torch.tensor(up, device=dev), x, opts)
        torch.cuda.synchronize()
    finally:
        if env and before is None:
            os.environ.pop(env, None)
        elif env:
            os.environ[env] = before
    res = {k: out[k].cpu().numpy() for k in KEYS if k != "x"}
    res["x"] = x.cpu().numpy()
    return res
