"""Diagnostic (not a test): rate of ntg_batch_envelope's entry envelope on config M (6 outputs, order 6, 20 intervals, 18 flag entries) at
nsub 0 and 2 -- problems/s and the achieved HBM rate on the bytes it must move (8 nC read + 2 x 8 x nz x npc written per problem) --
against a plain device-to-device copy that moves the same bytes (the yardstick of tools/copy_roof.py).  4096 problems is the size callers ask about (94 MB of
entry envelope at nsub 2) and runs for tens of microseconds, so a second, larger batch shows the rate once the call is long enough to be
throughput bound.  One JSON line at the end.
python tools/envelope_rate.py [batch ...]"""
import json
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntg_amd import api, configs as cf

batches = [int(a) for a in sys.argv[1:]] or [4096, 65536]
spec = cf.config_M()
plan = api.Plan(spec, 0)
L = api.lib()


def rate(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


res = dict(tool="envelope_rate", config="M", nC=spec.nC, nz=spec.nz)
for batch, nsub in [(b, n) for b in batches for n in (0, 2)]:
    x = torch.randn((batch, spec.nC), dtype=torch.float64, device="cuda:0")
    npc = max(spec.kninterv) << nsub
    lo = torch.empty((batch, spec.nz, npc), dtype=torch.float64, device="cuda:0"); hi = torch.empty_like(lo)
    st = plan._stream()

    def call():   # the C entry point on preallocated outputs: the allocation is not the kernel's
        rc = L.ntg_batch_envelope(plan.h, batch, x.data_ptr(), nsub, None, None, lo.data_ptr(), hi.data_ptr(), None, None, None, None, st)
        assert rc == 0, L.ntg_last_error().decode()
    nbytes = 8 * batch * (spec.nC + 2 * spec.nz * npc)
    ms = rate(call)
    a = torch.randn(nbytes // 16, dtype=torch.float64, device="cuda:0"); b = torch.empty_like(a)
    ms_copy = rate(lambda: b.copy_(a))
    print("envelope nsub %d: %d problems, npc %d (%.3f GB read + written): %.3f ms, %.0f problems/s, %.0f GB/s; copy of the same bytes %.3f ms, %.0f GB/s -> %.2f of the copy's rate"
          % (nsub, batch, npc, nbytes / 1e9, ms, batch / ms * 1e3, nbytes / ms / 1e6, ms_copy, nbytes / ms_copy / 1e6, ms_copy / ms))
    res["batch%d_nsub%d" % (batch, nsub)] = dict(npc=npc, bytes=nbytes, ms=round(ms, 4), problems_per_s=round(batch / ms * 1e3), gbps=round(nbytes / ms / 1e6, 1),
                                copy_ms=round(ms_copy, 4), copy_gbps=round(nbytes / ms_copy / 1e6, 1), of_copy=round(ms_copy / ms, 3))
    del a, b, lo, hi, x
print(json.dumps(res))
