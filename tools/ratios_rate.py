"""Diagnostic (not a test): ntg_batch_ratios of the squared curvature kappa^2 = T T / (S S S) of the kinematic car on the shapes of the tests'
cases at a batch of a few thousand, next to ntg_batch_forms of the two underlying forms S and T on the same batch: the loose steering bound
needs those two, the tight one the ratio.  Reported per case: problems/s of both calls, the mean of npieces (pairs per ratio, polygons per
form) and the share that ends with status OK.  The ratio is timed at 1e-9 of the largest quotient of the first 64 problems (what a planner
would ask for) and at the tests' tolerance (ratios_oracle.TOL_SLACKS slacks); the forms at forms_rate's tolerance.

  K4 / K20  kincar, order 6, 4 / 20 knot intervals.  Cars drive x = 8 t, y = 0.5, both perturbed, as in the tests.
One JSON line at the end.  No threshold: nothing exists to compare a new call's speed against.
python tools/ratios_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forms_oracle as fo
import ratios_oracle as ro
from ntg_amd import api, configs as cf, forms as fm

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = api.lib()


def rate(fn, reps=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


res = dict(tool="ratios_rate", batch=batch)
for name in ("K4", "K20"):
    l = 20 if name == "K20" else 4
    spec = cf._kincar_spec(1, 6, 3, l, 5 * l + 1, 5.0, f"kincar-2out-k6-l{l}")
    xh = fo.kincar_x(spec, batch, 191, *((0.1, 0.3) if name == "K20" else (0.2, 1.5)))
    forms, kappa2 = fm.curvature2(spec, (0, 1))
    head = ro.Inputs(name, spec, xh[:64], forms, [kappa2]).finish()
    big = max(r["rmax"] for row in head.levels() for r in row)
    ftol = max(1e-9 * max(float(np.abs(P).max()) for P in head.fpolys), 64.0 * float(head.fsl.max()))
    plan = api.Plan(spec, 0)
    x = torch.from_numpy(xh).to("cuda:0")
    nt = (api.C.c_int * 2)(*[len(f) for f in forms])
    flat = [api.FormTerm(*t) for f in forms for t in f]
    terms = (api.FormTerm * len(flat))(*flat)
    pad = lambda v: (api.C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))
    rat = (api.Ratio * 1)(api.Ratio(len(kappa2[0]), len(kappa2[1]), pad(kappa2[0]), pad(kappa2[1])))
    ext = torch.empty((batch, 2, 4), dtype=torch.float64, device="cuda:0")
    status = torch.empty((batch, 2), dtype=torch.int32, device="cuda:0"); npieces = torch.empty_like(status)
    st = plan._stream()

    def call_forms():   # the C entry points on preallocated outputs: the allocation is not the kernel's
        rc = L.ntg_batch_forms(plan.h, batch, x.data_ptr(), 2, nt, terms, 0, None, ftol, 30, 3, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    def call_ratio(tol):
        rc = L.ntg_batch_ratios(plan.h, batch, x.data_ptr(), 2, nt, terms, 0, None, 1, rat, tol, 30, 3, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    out = dict()
    ms = rate(call_forms)
    torch.cuda.synchronize()
    out["forms"] = dict(tol=ftol, ms=round(ms, 4), problems_per_s=round(batch / ms * 1e3), npieces_mean=round(float(npieces.cpu().numpy().mean()), 1), status_ok=float((status.cpu().numpy() == 0).mean()))
    for label, tol in (("fine", 1e-9 * big), ("tests", float(head.tol[0]))):
        ms = rate(lambda: call_ratio(tol))
        torch.cuda.synchronize()
        s, k = status.cpu().numpy().reshape(-1)[:batch], npieces.cpu().numpy().reshape(-1)[:batch]   # (one ratio: [batch][1] lies at the front of the buffers)
        out["kappa2_" + label] = dict(tol=tol, ms=round(ms, 4), problems_per_s=round(batch / ms * 1e3), npieces_mean=round(float(k.mean()), 1), npieces_max=int(k.max()),
                                      status_ok=float((s == 0).mean()), status_counts={int(v): int((s == v).sum()) for v in np.unique(s)})
    res[name] = out
    for k, v in out.items():
        print("%s, %s: %d problems in %.4f ms = %.3g problems/s; %.1f polygons (pairs) each, status OK %.3f" % (name, k, batch, v["ms"], v["problems_per_s"], v["npieces_mean"], v["status_ok"]))
print(json.dumps(res))
