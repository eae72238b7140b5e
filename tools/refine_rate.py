"""Diagnostic (not a test): HBM rate of ntg_batch_refine on config M's class (10 -> 20 intervals: 8 (nC_from + nC_to) bytes per problem)
against a plain device-to-device copy that moves the same bytes (the yardstick of tools/copy_roof.py).  python tools/refine_rate.py [batch]"""
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntg_amd import api, configs as cf

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
sc, sf = cf._kincar_spec(3, 6, 3, 10, 101, 5.0, "M on 10 intervals"), cf.config_M()
pc, pf = api.Plan(sc, 0), api.Plan(sf, 0)
x = torch.randn((batch, sc.nC), dtype=torch.float64, device="cuda:0")
nbytes = 8 * batch * (sc.nC + sf.nC)


def rate(fn, reps=10):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ms = rate(lambda: pc.refine(pf, x))
a = torch.randn(nbytes // 16, dtype=torch.float64, device="cuda:0"); b = torch.empty_like(a)
ms_copy = rate(lambda: b.copy_(a))
print("refine %d problems, nC %d -> %d (%.3f GB read + written): %.3f ms, %.0f GB/s" % (batch, sc.nC, sf.nC, nbytes / 1e9, ms, nbytes / ms / 1e6))
print("copy of the same bytes: %.3f ms, %.0f GB/s  ->  refine reaches %.2f of the copy's rate" % (ms_copy, nbytes / ms_copy / 1e6, ms_copy / ms))
