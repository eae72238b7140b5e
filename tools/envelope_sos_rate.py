"""Diagnostic (not a test): rate of ntg_batch_envelope_sos on config O (one obstacle row, order 6, 20 intervals: products of degree 10) and on
config D (thrust^2 and speed^2, order 8, 40 intervals: products of degree 10 and 12, the KM = 10 instance) at nsub 0 and 2 -- time per
call, problems/s, time per (row, piece) and the rate of the bytes it stores (2 x 8 x nnltc x npc per problem, plus 8 nC read).  For
comparison ntg_batch_envelope's row path (an existing kernel, not the code under test) on the plan of tests/cert_common.py's
rows_spec() -- kincar, order 6, 20 intervals, three linear rows y, x', x' - y' + 0.5 y'' -- at the same batch and nsub, and the ratio of
the two per (row, piece).  One JSON line at the end.
python tools/envelope_sos_rate.py [batch]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cert_common import rows_spec   # the tests' plan with three linear rows
from ntg_amd import api, configs as cf

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
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


def measure(name, spec, nsub, sos):
    plan = api.Plan(spec, 0)
    nrow = spec.nnltc if sos else spec.nltc
    npc = max(spec.kninterv) << nsub
    x = torch.randn((batch, spec.nC), dtype=torch.float64, device="cuda:0")
    lo = torch.empty((batch, nrow, npc), dtype=torch.float64, device="cuda:0"); hi = torch.empty_like(lo)
    st = plan._stream()

    def call():   # the C entry point on preallocated outputs: the allocation is not the kernel's
        if sos:
            rc = L.ntg_batch_envelope_sos(plan.h, batch, x.data_ptr(), nsub, None, None, lo.data_ptr(), hi.data_ptr(), None, None, st)
        else:
            rc = L.ntg_batch_envelope(plan.h, batch, x.data_ptr(), nsub, None, None, None, None, lo.data_ptr(), hi.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()
    ms = rate(call)
    stored = 16 * batch * nrow * npc
    ns_rp = ms * 1e6 / (batch * nrow * npc)
    print("%-8s nsub %d: %d problems, %d rows x %d pieces: %.4f ms, %.0f problems/s, %.4f ns per (row, piece), %.1f MB stored at %.0f GB/s"
          % (name, nsub, batch, nrow, npc, ms, batch / ms * 1e3, ns_rp, stored / 1e6, stored / ms / 1e6))
    return dict(rows=nrow, npc=npc, ms=round(ms, 4), problems_per_s=round(batch / ms * 1e3), ns_per_row_piece=round(ns_rp, 5), stored_bytes=stored,
                stored_gbps=round(stored / ms / 1e6, 1))


res = dict(tool="envelope_sos_rate", batch=batch)
for nsub in (0, 2):
    lin = measure("linear", rows_spec(), nsub, False)
    res["linear_nsub%d" % nsub] = lin
    for name, spec in (("O", cf.config_O()), ("D", cf.config_D())):
        r = measure("sos " + name, spec, nsub, True)
        r["per_row_piece_vs_linear"] = round(r["ns_per_row_piece"] / lin["ns_per_row_piece"], 2)
        print("         -> %.2f x the linear-row path per (row, piece)" % r["per_row_piece_vs_linear"])
        res["%s_nsub%d" % (name, nsub)] = r
print(json.dumps(res))
