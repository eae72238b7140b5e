"""ntg_batch_cost next to ntg_batch_check (no d_rows) on the same plan, batch and times.

The two kernels stage the same tile tables and coefficient rows and build the same flag in registers; the check evaluates the rows and
keeps a keyed maximum, the cost evaluates the family's running cost and keeps a weighted sum.  Case: config_M (kincar, 6 outputs) with a
linear ceiling row per car -- the plan tools/check_rate.py times as case M, the kincar family having no nonlinear rows for the check --
4096 problems, 1024 times (random coefficient vectors: the work does not depend on them).

    python tools/cost_rate.py [--batch 4096] [--ntimes 1024] [--reps 9] [--calls 200]
    python tools/cost_rate.py --resources       (no GPU: registers, LDS and scratch of every cost_kernel instance, from the saved assembly)

One warm-up window of each call, then --reps alternating windows of both, every window --calls back-to-back calls between two device
events; prints one JSON line with the medians per call, the window-to-window spreads (max - min), their ratio and the bytes each call
moves.  A record, not a gate."""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda:0"


def resources():
    """per cost_kernel instance of the library's units and the in-tree modules: the kernel descriptor's register, LDS and scratch fields"""
    out = {}
    pats = [os.path.join(ROOT, "ntg_amd", "csrc", "*gfx950.s"), os.path.join(ROOT, "ntg_amd", "modules", "*gfx950.s")]
    for path in sorted(p for pat in pats for p in glob.glob(pat)):
        cur = None
        for line in open(path, errors="replace"):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = None
                if re.match(r"_Z\d+cost_(kernel|final_kernel)", m.group(1)):
                    cur = os.path.basename(path).split("-hip-")[0] + ":" + m.group(1)
                    out[cur] = {}
                continue
            if cur and ".end_amdhsa_kernel" in line:
                cur = None
            if cur:
                m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)", line)
                if m:
                    out[cur][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ntimes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        for k, v in resources().items():
            print(json.dumps(dict(kernel=k, **v)))
        return
    import torch
    from ntg_amd import api
    from check_rate import case_spec
    if not torch.cuda.is_available():
        raise SystemExit("cost_rate.py measures on the GPU: none found")
    spec, bounds = case_spec("M")
    nb, nt = a.batch, a.ntimes
    plan = api.Plan(spec, 0)
    rng = np.random.default_rng(1)
    x = torch.tensor(rng.normal(size=(nb, spec.nC)), device=DEV)
    lo, up = (torch.tensor(np.ascontiguousarray(v), device=DEV) for v in bounds(nb))
    k0 = np.asarray(spec.knots[0])
    tn = np.clip(np.linspace(k0[0], k0[-1], nt), k0[0], k0[-1])
    times = torch.tensor(tn, device=DEV)
    weights = torch.tensor(np.gradient(tn), device=DEV)   # any weights: the work does not depend on them

    def timed(fn):
        """ms per call over a window of --calls back-to-back calls between two device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls, r
    run_cost = lambda: plan.cost(x, times, weights)
    run_check = lambda: plan.check(x, lo, up, times)
    timed(run_cost); timed(run_check)   # warm-up: code objects, the allocator's pools
    tc, tk = [], []
    for _ in range(max(a.reps, 5)):
        tc.append(timed(run_cost)[0]); tk.append(timed(run_check)[0])
    mc, mk = float(np.median(tc)), float(np.median(tk))
    kd = spec.order[0] * spec.maxderiv[0]
    ntab = nt * (kd * 8 + 4)                                  # the time tables (one basis class): written once, read once
    rd = nb * spec.nC * 8
    ntiles = (nt + 127) // 128
    by_cost = rd + 2 * ntab + 2 * nt * 8 + nb * 8 + 2 * nb * ntiles * 8
    by_check = rd + 2 * ntab + 2 * nb * spec.nbounds * 8 + nb * (8 + 8) + 2 * nb * ntiles * 16
    print(json.dumps(dict(spec=spec.name, batch=nb, ntimes=nt, calls_per_window=a.calls, cost_ms=round(mc, 4), check_ms=round(mk, 4),
                          cost_spread_ms=round(max(tc) - min(tc), 4), check_spread_ms=round(max(tk) - min(tk), 4),
                          cost_over_check=round(mc / mk, 3), cost_bytes=by_cost, check_bytes=by_check,
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
