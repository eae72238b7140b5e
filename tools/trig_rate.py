"""Diagnostic (not a test): ntg_batch_trig on the full manipulator plan (config E: 12 outputs, order 6, 60 knot intervals), 1024 problems, the
four tip-height forms sin qa + sin(qa + qb) + sin(qa + qb + qc), at tol 1e-6 and 1e-9.  Every arm swings as manipulator_bounds has it,
perturbed (tests/trig_oracle.py: arm_x).  Reported per tolerance: the median time of a call over 9 windows with the spread of the windows,
forms/s, the mean of npieces per form and the share of forms that end with status OK.  The yardstick printed next to it is Plan.check at
1001 times on the same plan and coefficients: samples only, no statement between them.  One JSON line at the end.
python tools/trig_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trig_oracle as to          # the tests' coefficients
from ntg_amd import api, configs as cf, trig as tg

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
L = api.lib()


def windows(fn, nwin=9, reps=10):
    """(median, smallest, largest) of the windows' times per call in ms"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


spec = cf.config_E()
narms = spec.nout // 3
plan = api.Plan(spec, 0)
xh = to.arm_x(spec, batch, 201)
x = torch.from_numpy(xh).to("cuda:0")
forms = [tg.tip_height(spec, a) for a in range(narms)]
nform = len(forms)
nt = (api.C.c_int * nform)(*[len(f) for f in forms])
pad = lambda v, ty: (ty * 4)(*(list(v) + [0] * (4 - len(v))))
flat = [api.TrigTerm(q.kind, len(q.ent), q.pp, 0, pad(q.ent, api.C.c_int), pad(q.coef, api.C.c_double), q.phase, q.w) for f in forms for q in f]
terms = (api.TrigTerm * len(flat))(*flat)
ext = torch.empty((batch, nform, 4), dtype=torch.float64, device="cuda:0")
status = torch.empty((batch, nform), dtype=torch.int32, device="cuda:0"); npieces = torch.empty_like(status)
st = plan._stream()
res = dict(tool="trig_rate", batch=batch, nform=nform)
for tol in (1e-6, 1e-9):
    def call():   # the C entry point on preallocated outputs: the allocation is not the kernel's
        rc = L.ntg_batch_trig(plan.h, batch, x.data_ptr(), nform, nt, terms, 0, None, tol, 30, 3, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    med, lo, hi = windows(call)
    s, k = status.cpu().numpy(), npieces.cpu().numpy()
    res["tol_%g" % tol] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), forms_per_s=round(batch * nform / med * 1e3), npieces_mean=round(float(k.mean()), 1),
                               npieces_max=int(k.max()), status_ok=float((s == 0).mean()))
    print("ntg_batch_trig, E, tol %g: %d problems x %d forms in %.4f ms (windows %.4f .. %.4f) = %.3g forms/s; %.1f pieces per form (most %d), status OK %.3f"
          % (tol, batch, nform, med, lo, hi, batch * nform / med * 1e3, k.mean(), k.max(), (s == 0).mean()))

lo_b, up_b = cf.manipulator_bounds(batch, narms=narms)
lo_d, up_d = torch.from_numpy(lo_b).to("cuda:0"), torch.from_numpy(up_b).to("cuda:0")
times = torch.linspace(0.0, 5.0, 1001, dtype=torch.float64, device="cuda:0")
med, lo, hi = windows(lambda: plan.check(x, lo_d, up_d, times))
res["check_1001"] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
print("Plan.check at 1001 times, the same plan and coefficients (samples only): %.4f ms a call (windows %.4f .. %.4f)" % (med, lo, hi))
print(json.dumps(res))
