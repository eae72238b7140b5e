"""The cases of tests/test_gpu_sqp_golden.py, shared with tools/record_wave_golden.py --sqp (which records the fixture
tests/golden/sqp_modes.npz): the structured Newton mode (hessian = 2) and the QP-based SQP step (hessian = 3) of sqp_kernel from x = 1, with
the bounds of tests/test_gpu_newton.py::_case, at the smallest shape at which each code path of the two modes exists:
  O        8 problems   one coupling group, small workgroup, 16 slots
  D2       4            a free output (the quadrotor's yaw)
  E2       4            several groups
  D        2            the two-sided factorisation (needs 128 free coefficients per group), 32 slots
  E        2            the BIG layout and the tuned manipulator instances (only the full size reaches them)
  O_warm   8            hessian = 3 twice on one plan and one workspace, the second solve with warm_start = 1 (no pass on the objective alone)
  Og, D8g  4            per-problem grids (tests/test_gpu_grids.py): the per-problem strides of the cost model and the free outputs' factors
  B        8            hessian = 2 on a plan without nonlinear rows: runs as hessian = 1
Every solve returns the multipliers (want_lambda) and runs a second time with NTG_AMD_STAMPS=3, which puts the modes' work counters
(factorisations, failures, solves, outer passes, majors, evaluations, passive-set solves, columns, full working sets, fallbacks, table columns)
into the first entries of each problem's multiplier row."""
import os

import numpy as np
import torch

from ntg_amd import api, configs as cf

KEYS = ("x", "objective", "inform", "iters", "nfev", "clambda", "counters")
NCOUNT = 11


def _d8_grids(spec, nb):
    """horizons in [0.9, 1.3] x the plan's (shorter flights violate the thrust bound outright), as tests/test_gpu_grids.py makes them"""
    from test_gpu_grids import grids_for
    knots, bps = grids_for(spec, nb, warp=0.1, seed=9)
    s0 = knots[:, :1]; sc = 0.9 + 0.4 * (knots[:, -1:] - s0 - 0.6 * 5.0) / 5.0
    knots = s0 + (knots - s0) / (knots[:, -1:] - s0) * 5.0 * sc; bps = s0 + (bps - s0) / (bps[:, -1:] - s0) * 5.0 * sc
    k0 = np.asarray(spec.knots[0]); l = spec.kninterv[0]
    j = np.minimum(np.searchsorted(k0, spec.bps, side="right") - 1, l - 1); inner = j < l - 1
    for b in range(nb):   # the affine map rounds: every breakpoint stays in the plan's knot interval in floating point
        bps[b] = np.maximum(bps[b], knots[b][j])
        bps[b][inner] = np.minimum(bps[b][inner], np.nextafter(knots[b][j + 1][inner], -np.inf))
        if spec.bps[-1] >= k0[-1]: bps[b][-1] = max(bps[b][-1], knots[b][-1])
    return knots, bps


def _o_grids(spec, nb):
    from test_gpu_grids import grids_for
    return grids_for(spec, nb, warp=0.2, seed=9)


_E2 = (lambda: cf.config_E(ninterv=20, narms=2), lambda n: cf.manipulator_bounds(n, narms=2))
# shape -> (spec, bounds, problems, per-problem grids or None)
SHAPES = {
    "O": (cf.config_O, cf.obstacle_bounds, 8, None),
    "D2": (lambda: cf.config_D(ninterv=10), cf.quadrotor_bounds, 4, None),
    "E2": _E2 + (4, None),
    "D": (cf.config_D, cf.quadrotor_bounds, 2, None),
    "E": (cf.config_E, cf.manipulator_bounds, 2, None),
    "Og": (cf.config_O, cf.obstacle_bounds, 4, _o_grids),
    "D8g": (lambda: cf.config_D(ninterv=8), cf.quadrotor_bounds, 4, _d8_grids),
    "B": (cf.config_B, lambda n: cf.kincar_random_bounds(1, n), 8, None),
}
# name -> (shape, hessian, warm: the recorded solve is a second one with warm_start = 1 on the first one's workspace)
CASES = {"%s_h%d" % (s, h): (s, h, False) for s in ("O", "D2", "E2", "D", "E", "Og", "D8g") for h in (2, 3)}
CASES["O_warm_h3"] = ("O", 3, True)
CASES["B_h2"] = ("B", 2, False)


def _solve(plan, spec, lo, up, hessian, warm, stamps):
    """one recorded solve from x = 1 (warm: behind a cold solve that leaves its multipliers in the workspace); NTG_AMD_STAMPS is read at every solve"""
    dev = torch.device("cuda:0")
    nb = lo.shape[0]
    cold, opts = api.default_opts(hessian=hessian), api.default_opts(hessian=hessian, warm_start=1 if warm else 0)
    work = torch.zeros(plan.workspace_bytes(nb, opts), dtype=torch.uint8, device=dev)
    lo_d, up_d = torch.tensor(lo, device=dev), torch.tensor(up, device=dev)
    if warm:
        plan.solve(lo_d, up_d, torch.ones((nb, spec.nC), dtype=torch.float64, device=dev), cold, work=work)
    x = torch.ones((nb, spec.nC), dtype=torch.float64, device=dev)
    before = os.environ.get("NTG_AMD_STAMPS")
    if stamps:
        os.environ["NTG_AMD_STAMPS"] = "3"
    else:
        os.environ.pop("NTG_AMD_STAMPS", None)
    try:
        out = plan.solve(lo_d, up_d, x, opts, work=work, want_lambda=True)
        torch.cuda.synchronize()
    finally:
        if before is None:
            os.environ.pop("NTG_AMD_STAMPS", None)
        else:
            os.environ["NTG_AMD_STAMPS"] = before
    res = {k: out[k].cpu().numpy() for k in ("objective", "inform", "iters", "nfev", "clambda")}
    res["x"] = x.cpu().numpy()
    return res


def run_case(name):
    """solve the case on cuda:0 with the loaded library; ({key: numpy array} for KEYS, the kernel the plan names for the solve)"""
    shape, hessian, warm = CASES[name]
    mk, bounds, nb, grids = SHAPES[shape]
    spec = mk()
    lo, up = bounds(nb)
    lo, up = np.ascontiguousarray(lo), np.ascontiguousarray(up)
    plan = api.Plan(spec, 0)
    if grids:
        kn, bp = grids(spec, nb)
        plan.set_grids(torch.tensor(kn, device="cuda:0"), torch.tensor(bp, device="cuda:0"), with_precond=True)
    kernel = plan.solve_kernel(nb, api.default_opts(hessian=hessian, warm_start=1 if warm else 0))
    res = _solve(plan, spec, lo, up, hessian, warm, False)
    counted = _solve(plan, spec, lo, up, hessian, warm, True) if shape != "B" else res   # (B runs another kernel: no counters of the modes)
    for k in ("x", "objective", "inform", "iters", "nfev"):   # (the counters change nothing but the rows they are written to)
        assert np.array_equal(res[k], counted[k]), k
    res["counters"] = np.ascontiguousarray(counted["clambda"][:, :NCOUNT])
    return res, kernel
