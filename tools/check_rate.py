"""ntg_batch_check next to ntg_batch_interp on the same plan, batch and times.

interp does the same basis products and writes every flag to HBM ([batch][ntimes][nz] doubles); the fused check evaluates the rows on
the flag in registers and writes a violation and its (row, time) per problem.  Cases (random coefficient vectors: the work does not
depend on them):

  O   config_O (kincar, 2 outputs, one obstacle row)                 --batch 4096 --ntimes 1001
  M   config_M (kincar, 6 outputs) with a linear ceiling row per car   --batch 4096 --ntimes 1001
      (the obstacle families take two outputs only, so the 6-output case checks linear trajectory rows)
  E   config_E (manipulator, 12 outputs, 4 tip-height rows)          --batch 1024 --ntimes 1001

    python tools/check_rate.py --case O [--batch N] [--ntimes N] [--reps 9] [--calls 200] [--grids]
    python tools/check_rate.py --resources       (no GPU: registers, LDS and scratch of every check_kernel instance, from the saved assembly)

One warm-up window of each call, then --reps alternating windows of both, every window --calls back-to-back calls between two device
events (a single call of a few tenths of a millisecond would time the clock and the scheduler); prints one JSON line with the medians
per call, the window-to-window spreads (max - min), the bytes each call moves and the verdict of DESIGN.md §2c (check <= interp + the larger spread).
--grids puts every problem on its own horizon (per-problem grids, per-problem times).  Run every case as a process of its own, under
its own time limit."""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def resources():
    """per check_kernel instance of the library's units and the in-tree modules: the kernel descriptor's register, LDS and scratch fields"""
    out = {}
    pats = [os.path.join(ROOT, "ntg_amd", "csrc", "*gfx950.s"), os.path.join(ROOT, "ntg_amd", "modules", "*gfx950.s")]
    for path in sorted(p for pat in pats for p in glob.glob(pat)):
        cur = None
        for line in open(path, errors="replace"):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = m.group(1) if "check_kernel" in m.group(1) or "check_final" in m.group(1) else None
                if cur:
                    out[os.path.basename(path).split("-hip-")[0] + ":" + cur] = {}
                    cur = os.path.basename(path).split("-hip-")[0] + ":" + cur
                continue
            if cur and ".end_amdhsa_kernel" in line:
                cur = None
            if cur:
                m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)", line)
                if m:
                    out[cur][m.group(1)] = int(m.group(2))
    return out


def case_spec(name):
    from ntg_amd import configs as cf
    if name == "O":
        return cf.config_O(), cf.obstacle_bounds
    if name == "M":
        s = cf.config_M()   # the kincar family has no nonlinear rows: one linear trajectory row per car, a ceiling on its y
        ltc = np.zeros((3, s.nz))
        for c in range(3):
            ltc[c, 6 * c + 3] = 1.0
        s.ltc = ltc; s.lin_ineq = [0] * 18 + [1] * 3 + [0] * 18; s.name = "M+ceilings"

        def bounds(nb):
            lo, up = cf.kincar_random_bounds(3, nb)
            top = np.maximum(lo[:, 3:18:6], lo[:, 21:36:6]) + 0.05
            return (np.concatenate([lo[:, :18], np.full((nb, 3), -cf.INF_BOUND), lo[:, 18:]], axis=1),
                    np.concatenate([up[:, :18], top, up[:, 18:]], axis=1))
        return s, bounds
    if name == "E":
        return cf.config_E(), lambda nb: cf.manipulator_bounds(nb, narms=4)
    raise SystemExit("unknown case " + name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="O")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--ntimes", type=int, default=1001)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--grids", action="store_true")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        for k, v in resources().items():
            print(json.dumps(dict(kernel=k, **v)))
        return
    import torch
    from ntg_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("check_rate.py measures on the GPU: none found")
    spec, bounds = case_spec(a.case)
    nb = a.batch or (1024 if a.case == "E" else 4096)
    nt = a.ntimes
    plan = api.Plan(spec, 0)
    rng = np.random.default_rng(1)
    x = torch.tensor(rng.normal(size=(nb, spec.nC)), device=DEV)
    lo, up = (torch.tensor(np.ascontiguousarray(v), device=DEV) for v in bounds(nb))
    k0 = np.asarray(spec.knots[0])
    if a.grids:
        scale = rng.uniform(0.6, 1.6, nb)
        kn = k0[None, :] * scale[:, None]; bp = np.asarray(spec.bps)[None, :] * scale[:, None]
        bp = np.minimum(bp, kn[:, -1:])
        plan.set_grids(torch.tensor(kn, device=DEV), torch.tensor(bp, device=DEV), with_precond=False)
        times = torch.tensor(np.minimum(np.linspace(0.0, 1.0, nt)[None, :] * kn[:, -1:], kn[:, -1:]), device=DEV)
    else:
        times = torch.tensor(np.clip(np.linspace(k0[0], k0[-1], nt), k0[0], k0[-1]), device=DEV)

    def timed(fn):
        """ms per call over a window of --calls back-to-back calls between two device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls, r
    run_check = lambda: plan.check(x, lo, up, times)
    run_interp = lambda: plan.interp(x, times)
    timed(run_check); timed(run_interp)   # warm-up: code objects, the allocator's pools
    tc, ti = [], []
    for _ in range(max(a.reps, 5)):
        tc.append(timed(run_check)[0]); ti.append(timed(run_interp)[0])
    out = run_check()
    mc, mi = float(np.median(tc)), float(np.median(ti))
    sc, si = max(tc) - min(tc), max(ti) - min(ti)
    kd = sum(k * d for k, d in zip(spec.order[:1], spec.maxderiv[:1]))
    ntab = (nb if a.grids else 1) * nt * (kd * 8 + 4)                     # the time tables (one basis class in every case here): written once, read once
    rd = nb * spec.nC * 8
    by_interp = rd + 2 * ntab + nb * nt * spec.nz * 8
    by_check = rd + 2 * ntab + 2 * nb * spec.nbounds * 8 + nb * (8 + 8) + 2 * nb * ((nt + 127) // 128) * 16
    print(json.dumps(dict(case=a.case, spec=spec.name, batch=nb, ntimes=nt, per_problem_grids=bool(a.grids), calls_per_window=a.calls, lib=os.path.basename(os.path.dirname(api.LIB_PATH)),
                          check_ms=round(mc, 4), interp_ms=round(mi, 4), check_spread_ms=round(sc, 4), interp_spread_ms=round(si, 4),
                          check_bytes=by_check, interp_bytes=by_interp, check_not_slower=bool(mc <= mi + max(sc, si)),
                          problems_violating=int((out["viol"] > 0).sum()), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
