"""Diagnostic (not a test): ntg_batch_minmax on the kinematic-car plan of the benchmark's shape (config B: 2 outputs, order 6, 20 knot
intervals), 1024 problems that drive past x = 20 (tests/forms_oracle.py: kincar_x), at tol 1e-6: a square obstacle (4 members), an octagon
(8 members) and a corridor of three boxes (12 members, MIN of MAX), each one group of one call.  Reported per group: the median time of a
call over 9 windows with the spread of the windows, groups/s, the mean and the largest npieces and the share of status OK.  The yardstick
printed next to each is ntg_batch_forms over the same member forms on the same batch at the same tolerance: it does the same level-0 work,
but it bisects every member everywhere (the corridor's 12 forms take two calls of 8 and 4, timed together).  One JSON line at the end.
python tools/minmax_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forms_oracle as fo         # the tests' coefficients
import minmax_oracle as mo
from ntg_amd import api, configs as cf, minmax as mm

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
tol = 1e-6
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


def declare(forms):
    nt = (api.C.c_int * len(forms))(*[len(f) for f in forms])
    flat = [api.FormTerm(*t) for f in forms for t in f]
    return nt, (api.FormTerm * len(flat))(*flat)


spec = cf.config_B()
plan = api.Plan(spec, 0)
x = torch.from_numpy(fo.kincar_x(spec, batch, 301)).to("cuda:0")
st = plan._stream()
cases = {"square": mm.box(spec, 0, 1, 20.0, 0.5, 2.0, 2.0),
         "octagon": mm.polygon(spec, 0, 1, mo.ngon(8, 20.0, 0.5, 3.0)),
         "corridor3": mm.corridor(spec, 0, 1, [(8.0, 0.5, 10.0, 4.0), (22.0, 0.0, 8.0, 5.0, 0.05), (34.0, 0.5, 8.0, 4.5)])}
ext = torch.empty((batch, 8, 4), dtype=torch.float64, device="cuda:0")
status = torch.empty((batch, 8), dtype=torch.int32, device="cuda:0"); npieces = torch.empty_like(status)
res = dict(tool="minmax_rate", batch=batch, tol=tol)
for name, (forms, (outer, inner, clauses)) in cases.items():
    nform = len(forms)
    nt, terms = declare(forms)
    grp = (api.MinmaxGroup * 1)(api.MinmaxGroup(outer, inner, len(clauses), 0, (api.C.c_int * 8)(*([len(c) for c in clauses] + [0] * (8 - len(clauses))))))
    mem = (api.MinmaxMember * nform)(*[api.MinmaxMember(f, pc, c) for cl in clauses for f, c, pc in cl])

    def call():   # the C entry point on preallocated outputs: the allocation is not the kernel's
        rc = L.ntg_batch_minmax(plan.h, batch, x.data_ptr(), nform, nt, terms, 0, None, 1, grp, mem, tol, 30, 3, None, None, ext.data_ptr(), None, None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    med, lo, hi = windows(call)
    s, k = status.cpu().numpy().reshape(-1)[:batch], npieces.cpu().numpy().reshape(-1)[:batch]   # [batch][1] in the front of the buffers
    parts = [declare(forms[a:a + 8]) + (len(forms[a:a + 8]),) for a in range(0, nform, 8)]

    def members():
        for pnt, pterms, n in parts:
            rc = L.ntg_batch_forms(plan.h, batch, x.data_ptr(), n, pnt, pterms, 0, None, tol, 30, 3, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
            assert rc == 0, L.ntg_last_error().decode()

    fmed, flo, fhi = windows(members)
    res[name] = dict(members=nform, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), groups_per_s=round(batch / med * 1e3), npieces_mean=round(float(k.mean()), 1),
                     npieces_max=int(k.max()), status_ok=float((s == 0).mean()), forms_ms=round(fmed, 4), forms_ms_min=round(flo, 4), forms_ms_max=round(fhi, 4),
                     ratio=round(med / fmed, 3))
    print("ntg_batch_minmax, B, %s (%d members), tol %g: %d problems in %.4f ms (windows %.4f .. %.4f) = %.3g groups/s; %.1f pieces per group (most %d), status OK %.3f"
          % (name, nform, tol, batch, med, lo, hi, batch / med * 1e3, k.mean(), k.max(), (s == 0).mean()))
    print("    ntg_batch_forms over the same %d member forms: %.4f ms (windows %.4f .. %.4f); minmax / forms = %.2f" % (nform, fmed, flo, fhi, med / fmed))
print(json.dumps(res))
