"""Diagnostic (not a test): what a coarse-to-fine cascade costs against a cold solve, on config M's kincar class (3 cars, order 6, 101
breakpoints) with the product-default preconditioned solve (hessian = 1), to convergence.
  (a) cold solve on 20 intervals from x = 1
  (b) solve on 10 intervals from x = 1, ntg_batch_refine onto 20 intervals, solve on 20 from the refined start
Prints time and majors of every leg.  python tools/cascade_rate.py [batch]"""
import os
import sys
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntg_amd import api, configs as cf

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
sc, sf = cf._kincar_spec(3, 6, 3, 10, 101, 5.0, "M on 10 intervals"), cf.config_M()
pc, pf = api.Plan(sc, 0), api.Plan(sf, 0)
lo, up = (torch.tensor(a, device="cuda:0") for a in cf.kincar_random_bounds(3, batch))
opts = api.default_opts(hessian=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
    return r, e0.elapsed_time(e1)


def ones(spec):
    return torch.ones((batch, spec.nC), dtype=torch.float64, device="cuda:0")


def report(leg, out, ms):
    it, inf = out["iters"].cpu().numpy(), out["inform"].cpu().numpy()
    print("%-34s %9.3f ms   majors mean %.2f max %d   inform 0: %d / %d   objective mean %.6f" %
          (leg, ms, it.mean(), it.max(), (inf == 0).sum(), batch, out["objective"].mean().item()))


for rep in range(2):   # the first pass builds the preconditioners and warms the kernels; the second is the measurement
    xa = ones(sf); a, ta = timed(lambda: pf.solve(lo, up, xa, opts))
    xc = ones(sc); c, tc = timed(lambda: pc.solve(lo, up, xc, opts))
    xr, tr = timed(lambda: pc.refine(pf, xc))
    b, tb = timed(lambda: pf.solve(lo, up, xr, opts))
    if rep == 0:
        continue
    print("batch %d, kernels: fine %s, coarse %s" % (batch, pf.solve_kernel(batch, opts), pc.solve_kernel(batch, opts)))
    report("(a) cold solve, 20 intervals", a, ta)
    report("(b1) solve, 10 intervals", c, tc)
    print("%-34s %9.3f ms" % ("(b2) refine 10 -> 20", tr))
    report("(b3) solve, 20 from refined start", b, tb)
    print("(b) total %.3f ms = %.2f x (a);  objective (b3) - (a): max |d| / |a| = %.2e" %
          (tc + tr + tb, (tc + tr + tb) / ta, ((b["objective"] - a["objective"]).abs() / a["objective"].abs()).max().item()))
