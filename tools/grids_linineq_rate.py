"""Per-problem grids on a plan with linear inequality rows: config B plus a ceiling on y at every breakpoint (one ltc row declared a range,
101 rows of the augmented Lagrangian), next to plain config B.

  set_grids   wall time of ntg_plan_set_grids for --grids horizons in [0.6, 1.6] x the plan's, with and without the ceiling row
  solve       hessian = 1 to convergence for --batch problems (kincar_random_bounds, ceiling 0.05 above both end points) on sqp_kernel: the
              shared grid; per-problem grids that all equal the plan's own (the same problems: only the tables' addressing differs);
              per-problem horizons (other problems, other iteration counts)

    python tools/grids_linineq_rate.py [--grids 16384] [--batch 4096] [--reps 5]
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntg_amd import api, configs as cf  # noqa: E402

DEV = "cuda:0"


def ceiling_spec():
    s = cf.config_B()
    ltc = np.zeros((1, s.nz)); ltc[0, 3] = 1.0
    s.ltc = ltc
    s.lin_ineq = [0] * 6 + [1] + [0] * 6
    return s


def horizons(spec, nb, seed=3):
    """nb uniform break sequences over [0.6, 1.6] x the plan's horizon, every breakpoint in the plan's knot interval (as tests/test_gpu_grids.grids_for)"""
    k0 = np.asarray(spec.knots[0]); l = spec.kninterv[0]
    kn = k0[None, :] * np.random.default_rng(seed).uniform(0.6, 1.6, nb)[:, None]
    j = np.minimum(np.searchsorted(k0, spec.bps, side="right") - 1, l - 1)
    fr = (np.asarray(spec.bps) - k0[j]) / (k0[j + 1] - k0[j])
    bp = kn[:, j] + fr[None, :] * (kn[:, j + 1] - kn[:, j])
    inner = j < l - 1
    bp = np.maximum(bp, kn[:, j]); bp[:, inner] = np.minimum(bp[:, inner], np.nextafter(kn[:, j + 1][:, inner], -np.inf))
    bp[:, -1] = np.maximum(bp[:, -1], kn[:, -1])
    return torch.tensor(np.ascontiguousarray(kn), device=DEV), torch.tensor(np.ascontiguousarray(bp), device=DEV)


def time_set_grids(plan, kn, bp, with_precond, reps):
    ts = []
    for _ in range(reps + 1):   # the first call uploads the plan's shared inputs once
        torch.cuda.synchronize(); t = time.perf_counter()
        plan.set_grids(kn, bp, with_precond=with_precond)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    plan.clear_grids()
    return round(1e3 * float(np.median(ts[1:])), 2)


def time_solve(plan, lo, up, o, reps):
    nb = lo.shape[0]
    lo, up = torch.tensor(lo, device=DEV), torch.tensor(up, device=DEV)
    work = torch.empty(plan.workspace_bytes(nb, o), dtype=torch.uint8, device=DEV)
    times = []
    for r in range(reps + 1):   # the first run builds what the plan builds on first use
        x = torch.ones((nb, plan.spec.nC), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = plan.solve(lo, up, x, o, work=work)
        b.record()
        torch.cuda.synchronize()
        if r:
            times.append(a.elapsed_time(b) / 1e3)
    t = float(np.median(times))
    inform, iters = out["inform"].cpu().numpy(), out["iters"].cpu().numpy()
    return dict(ms=round(t * 1e3, 3), traj_per_s=round(nb / t), inform01=float(np.isin(inform, (0, 1)).mean()),
                mean_iters=round(float(iters.mean()), 2), kernel=plan.solve_kernel(nb, o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    plain, ceil = api.Plan(cf.config_B(), 0), api.Plan(ceiling_spec(), 0)
    kn, bp = horizons(plain.spec, a.grids)
    for wp in (False, True):
        tp = time_set_grids(plain, kn, bp, wp, a.reps)
        tc = time_set_grids(ceil, kn, bp, wp, a.reps)
        print(json.dumps(dict(what="set_grids", grids=a.grids, with_precond=wp, config_B_ms=tp, config_B_ceiling_ms=tc)), flush=True)
    nb = a.batch
    lo0, up0 = cf.kincar_random_bounds(1, nb)
    ymax = np.maximum(lo0[:, 3], lo0[:, 9]) + 0.05
    lo = np.concatenate([lo0[:, :6], np.full((nb, 1), -cf.INF_BOUND), lo0[:, 6:]], axis=1)
    up = np.concatenate([up0[:, :6], ymax[:, None], up0[:, 6:]], axis=1)
    o = api.default_opts(hessian=1, itlim=3000)
    shared = time_solve(ceil, lo, up, o, a.reps)
    own_k = torch.tensor(np.tile(np.asarray(ceil.spec.knots[0]), (nb, 1)), device=DEV)
    own_b = torch.tensor(np.tile(np.asarray(ceil.spec.bps), (nb, 1)), device=DEV)
    ceil.set_grids(own_k, own_b, with_precond=True)
    same = time_solve(ceil, lo, up, o, a.reps)
    kb, bb = horizons(ceil.spec, nb, seed=5)
    ceil.set_grids(kb, bb, with_precond=True)
    grids = time_solve(ceil, lo, up, o, a.reps)
    print(json.dumps(dict(what="solve", batch=nb, hessian=1, shared=shared, per_problem_copies_of_the_plans_grid=same, per_problem_horizons=grids,
                          copies_over_shared=round(same["traj_per_s"] / shared["traj_per_s"], 4),
                          horizons_over_shared=round(grids["traj_per_s"] / shared["traj_per_s"], 4))), flush=True)


if __name__ == "__main__":
    main()
