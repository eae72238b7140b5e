"""Time per call of ntg_batch_verify / Plan.verify on configs M, D and E and on the unicycle module.

The call evaluates every used callback slot 2 nz + 1 times per breakpoint (the analytic derivatives once, a central difference per flag
entry), all in registers for the narrow instances; the work does not depend on the coefficients, which are random here.

    python tools/verify_rate.py [--batch 1024] [--reps 7] [--calls 20]
    python tools/verify_rate.py --resources       (no GPU: registers, LDS and scratch of every verify_kernel instance, from the saved assembly)

One warm-up window per case, then --reps windows of --calls back-to-back calls between two device events; prints one JSON line per case
with the median per call, the window-to-window spread (max - min) and the callback evaluations per second it amounts to.  A record, not a
gate."""
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
    """per verify_kernel instance of the library's units and the in-tree modules: the kernel descriptor's register, LDS and scratch fields"""
    out = {}
    pats = [os.path.join(ROOT, "ntg_amd", "csrc", "*gfx950.s"), os.path.join(ROOT, "ntg_amd", "modules", "*gfx950.s")]
    for path in sorted(p for pat in pats for p in glob.glob(pat)):
        cur = None
        for line in open(path, errors="replace"):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = None
                if re.match(r"_Z\d+verify_(kernel|final_kernel)", m.group(1)):
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


def evaluations(spec):
    """callback evaluations per problem: (2 nz + 1) per audited point of every used slot"""
    P, per = spec.nbps, 2 * spec.nz + 1
    pts = (1 if spec.nicf else 0) + (P if spec.nucf else 0) + (1 if spec.nfcf else 0) + (1 if spec.nnlic else 0) + (P if spec.nnltc else 0) + (1 if spec.nnlfc else 0)
    return pts * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        for k, v in resources().items():
            print(json.dumps(dict(kernel=k, **v)))
        return
    import torch
    from ntg_amd import api, configs as cf, family
    if not torch.cuda.is_available():
        raise SystemExit("verify_rate.py measures on the GPU: none found")
    uni = api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))
    cases = [("M", cf.config_M()), ("D", cf.config_D()), ("E", cf.config_E()), ("U", cf.config_U(uni))]
    for name, spec in cases:
        plan = api.Plan(spec, 0)
        x = torch.tensor(0.3 * np.random.default_rng(1).normal(size=(a.batch, spec.nC)), device=DEV)

        def window():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                plan.verify(x)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.calls
        window()   # warm-up: code objects, the allocator's pools
        t = [window() for _ in range(max(a.reps, 3))]
        med = float(np.median(t))
        print(json.dumps(dict(case=name, spec=spec.name, batch=a.batch, nbps=spec.nbps, nz=spec.nz, calls_per_window=a.calls, verify_ms=round(med, 4),
                              spread_ms=round(max(t) - min(t), 4), evals_per_problem=evaluations(spec),
                              gevals_per_s=round(a.batch * evaluations(spec) / (med * 1e-3) / 1e9, 3), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
