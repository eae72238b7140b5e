"""Diagnostic (not a test): ntg_batch_extrema against the fixed subdivision it replaces, on config O (one obstacle row, order 6, 20
intervals) and config D (thrust^2 and speed^2, order 8, 40 intervals: the KM = 10 instance).  Per config: the time of ntg_batch_extrema
(sides = 1, tol = max(1e-9 max |value|, 64 slack) as in the tests), the time of ntg_batch_envelope_sos at nsub = 6 on the same inputs (an
existing kernel: the yardstick), the mean of npieces against the l * 64 polygons per row of the fixed subdivision, and the shares of rows
ending OK / FULL / DEPTH, and the width of the enclosure of the minimum both reach: min_hi - min_lo here (over the rows ending OK), min over
pieces of q_hi less min over pieces of q_lo there (over all rows).  One JSON line at
the end.
python tools/extrema_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extrema_oracle as xo   # the tests' inputs and slack
from ntg_amd import api, configs as cf

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = api.lib()
NSUB = 6


def rate(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(name, spec, xh):
    plan = api.Plan(spec, 0)
    nrow, l = spec.nnltc, max(spec.kninterv)
    x = torch.from_numpy(xh).to("cuda:0")
    slack = xo.slack(spec, xh)
    zero = plan.extrema(x, 0.0, max_depth=0)["ext"].cpu().numpy()
    tol = max(1e-9 * float(np.abs(zero).max()), 64.0 * float(slack.max()))
    ext = torch.empty((batch, nrow, 4), dtype=torch.float64, device="cuda:0")
    npieces = torch.empty((batch, nrow), dtype=torch.int32, device="cuda:0"); status = torch.empty_like(npieces)
    lo = torch.empty((batch, nrow, l << NSUB), dtype=torch.float64, device="cuda:0"); hi = torch.empty_like(lo)
    st = plan._stream()

    def call_ext():   # the C entry points on preallocated outputs: the allocation is not the kernel's
        rc = L.ntg_batch_extrema(plan.h, batch, x.data_ptr(), tol, 30, 1, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    def call_sos():
        rc = L.ntg_batch_envelope_sos(plan.h, batch, x.data_ptr(), NSUB, None, None, lo.data_ptr(), hi.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()
    ms_ext, ms_sos = rate(call_ext), rate(call_sos)
    torch.cuda.synchronize()
    e, n, s = ext.cpu().numpy(), npieces.cpu().numpy(), status.cpu().numpy()
    ok = s == 0
    w_ext = (e[..., 1] - e[..., 0])[ok]   # (a row stopped by FULL or DEPTH keeps a sound but wide enclosure: counted apart)
    w_sos = (hi.min(dim=2).values - lo.min(dim=2).values).cpu().numpy()
    r = dict(rows=nrow, l=l, tol=tol, ms_extrema=round(ms_ext, 4), ms_envelope_sos_nsub6=round(ms_sos, 4), speedup=round(ms_sos / ms_ext, 2),
             npieces_mean=round(float(n.mean()), 1), npieces_max=int(n.max()), fixed_pieces=l << NSUB, status_ok=float(ok.mean()), status_full=float((s == 2).mean()), status_depth=float((s == 1).mean()),
             width_extrema_mean=float(w_ext.mean()), width_extrema_max=float(w_ext.max()), width_sos_mean=float(w_sos.mean()), width_sos_max=float(w_sos.max()))
    print("%-2s %d problems, %d rows, l = %d: extrema %.4f ms (tol %.3g, %.1f polygons per row on average, at most %d, status OK %.3f, FULL %.3f), envelope_sos nsub 6 %.4f ms "
          "(%d polygons per row): %.2f x; width of the minimum's enclosure on the OK rows %.3g (max %.3g) against %.3g (max %.3g)"
          % (name, batch, nrow, l, ms_ext, tol, r["npieces_mean"], r["npieces_max"], r["status_ok"], r["status_full"], ms_sos, l << NSUB, r["speedup"], r["width_extrema_mean"],
             r["width_extrema_max"], r["width_sos_mean"], r["width_sos_max"]))
    return r


res = dict(tool="extrema_rate", batch=batch)
so_ = cf.config_O()
res["O"] = measure("O", so_, xo.obstacle_x(so_, batch, 81))
sd = cf.config_D()
res["D"] = measure("D", sd, np.random.default_rng(82).standard_normal((batch, sd.nC)))
print(json.dumps(res))
