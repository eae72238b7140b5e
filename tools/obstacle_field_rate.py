"""Trajectories per second of the obstacle-field family (NTG_FAM_OBSTACLE_FIELD, per-problem centres) next to the obstacle family
(NTG_FAM_OBSTACLE, one compile-time centre), 4096 problems, hessian = 3 (QP-based step, cold) and hessian = 2 (structured Newton).

  m = 1: the field family with every centre at (20, 0.5) and config_O's bounds -- the same problems, so the same work
  m = 4: four obstacles per problem on each problem's route (configs.obstacle_field_problems)

    python tools/obstacle_field_rate.py [--batch 4096] [--reps 5]
Prints one JSON line per (m, hessian)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntg_amd import api, configs as cf  # noqa: E402


def rate(plan, lo, up, x0, hessian, reps):
    dev = torch.device("cuda:0")
    lo, up = torch.tensor(lo, device=dev), torch.tensor(up, device=dev)
    o = api.default_opts(hessian=hessian)
    work = torch.empty(plan.workspace_bytes(x0.shape[0], o), dtype=torch.uint8, device=dev)
    times, inform = [], None
    for r in range(reps + 1):   # the first run builds what the plan builds on first use
        x = torch.tensor(x0, device=dev)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = plan.solve(lo, up, x, o, work=work)
        b.record()
        torch.cuda.synchronize()
        if r:
            times.append(a.elapsed_time(b) / 1e3)
        inform = out["inform"].cpu().numpy()
    t = float(np.median(times))
    return dict(ms=round(t * 1e3, 3), traj_per_s=round(x0.shape[0] / t), inform0=float((inform == 0).mean()), kernel=plan.solve_kernel(x0.shape[0], o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    nb = a.batch
    po = api.Plan(cf.config_O(), 0)
    lo1, up1 = cf.obstacle_bounds(nb)
    x0 = np.ones((nb, po.spec.nC))
    for m in (1, 4):
        pf = api.Plan(cf.config_OF(m), 0)
        if m == 1:
            prm, lo, up = np.tile([20.0, 0.5], (nb, 1)), lo1, up1
        else:
            prm, lo, up = cf.obstacle_field_problems(nb, m)
        pf.set_params(torch.tensor(prm, device="cuda:0"))
        for h in (3, 2):
            rf = rate(pf, lo, up, x0, h, a.reps)
            ro = rate(po, lo1, up1, x0, h, a.reps)
            print(json.dumps(dict(m=m, hessian=h, batch=nb, field=rf, obstacle=ro,
                                  field_over_obstacle=round(rf["traj_per_s"] / ro["traj_per_s"], 4))), flush=True)


if __name__ == "__main__":
    main()
