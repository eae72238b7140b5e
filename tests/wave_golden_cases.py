"""The cases of tests/test_gpu_wave_golden_instances.py, shared with tools/record_wave_golden.py (which records the fixture
tests/golden/wave_instances.npz): instances of sqp_wave_kernel other than the headline one, each solved for the first 8 problems of
cf.kincar_random_bounds(ncars, 4096) from x = 1 with the identity cold start.  Unless a case says otherwise it runs exactly 50
majors, so one solve passes through every chain length 2 .. 50 -- every boundary of the chain's tiers (registers, LDS, HBM)."""
import os

import numpy as np
import torch

from ntg_amd import api, configs as cf

NB = 8
FIXED50 = dict(itlim=50, fixed_iters=1, hessian=0)
KEYS = ("x", "objective", "inform", "iters", "nfev")


def _m4b():
    return cf._kincar_spec(2, 6, 3, 16, 81, 5.0, "M4b:kincar-4out-k6-l16")   # gpu_common's M4b


def scaled_grids(spec, nb):
    """nb horizons in [0.6, 1.6] x the plan's, breakpoints at the same relative places (bench.py: per_problem_grids)"""
    k0 = np.asarray(spec.knots[0])
    scale = np.random.default_rng(3).uniform(0.6, 1.6, nb)[:, None]
    kn = k0[None, :] * scale
    jj = np.minimum(np.searchsorted(k0, spec.bps, side="right") - 1, spec.kninterv[0] - 1)
    fr = (np.asarray(spec.bps) - k0[jj]) / (k0[jj + 1] - k0[jj])
    bpg = kn[:, jj] + fr[None, :] * (kn[:, jj + 1] - kn[:, jj])
    inner = jj < spec.kninterv[0] - 1
    bpg = np.maximum(bpg, kn[:, jj])
    bpg[:, inner] = np.minimum(bpg[:, inner], np.nextafter(kn[:, jj + 1][:, inner], -np.inf))
    bpg[:, -1] = kn[:, -1]
    return np.ascontiguousarray(kn), np.ascontiguousarray(bpg)


# name -> (spec, cars, solve options, environment variable to set or None, per-problem grids)
CASES = {
    "B_fixed50": (cf.config_B, 1, FIXED50, None, False),                                                   # 2 outputs, 3 doubles per lane, 40 register slots
    "G4_fixed50": (lambda: cf._kincar_spec(2, 6, 3, 20, 101, 5.0, "G4"), 2, FIXED50, None, False),          # 4 outputs on 20 intervals
    "M4b_fixed50": (_m4b, 2, FIXED50, None, False),                                                        # 4 outputs on 16 intervals: the other accumulator-base class
    "M_noagpr_fixed50": (cf.config_M, 3, FIXED50, "NTG_AMD_WAVE_NOAGPR", False),                            # no register slots: LDS tier first, 40 slots in HBM
    "M_grids_fixed50": (cf.config_M, 3, FIXED50, None, True),                                              # per-problem grids: two LDS slots
    "M_memory24_fixed50": (cf.config_M, 3, dict(FIXED50, qn_memory=24), None, False),                       # restarts at accepted steps, no HBM tier
    "M_to_convergence": (cf.config_M, 3, dict(hessian=0), None, False),                                    # long memory: the six-LDS-slot instance
}


def run_case(name):
    """solve the case on cuda:0 with the loaded library; {key: numpy array} for KEYS"""
    mk, ncars, kw, env, grids = CASES[name]
    spec = mk()
    lo, up = cf.kincar_random_bounds(ncars, 4096)
    lo, up = np.ascontiguousarray(lo[:NB]), np.ascontiguousarray(up[:NB])
    dev = torch.device("cuda:0")
    opts = api.default_opts(**kw)
    plan = api.Plan(spec, 0)
    # (the variable is read when the launch is planned -- at solve_kernel and solve time, not when the plan is made -- so it is set around
    # those calls only.  Nothing reports which instance ran: that NTG_AMD_WAVE_NOAGPR took effect shows in the fixture, whose
    # results for this case differ in the last bits from the headline instance's, the tiers adding the chain's terms in another order.)
    before = os.environ.get(env) if env else None
    if env:
        os.environ[env] = "1"
    try:
        if grids:
            kn, bpg = scaled_grids(spec, NB)
            plan.set_grids(torch.tensor(kn, device=dev), torch.tensor(bpg, device=dev), with_precond=False)
        kernel = plan.solve_kernel(NB, opts)
        assert kernel == "sqp_wave_kernel", kernel
        x = torch.ones((NB, spec.nC), dtype=torch.float64, device=dev)
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
