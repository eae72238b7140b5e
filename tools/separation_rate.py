"""Diagnostic (not a test): ntg_batch_separation on config M (three cars per problem, order 6, 20 intervals).  The pairs are the three pairs
of cars of every problem plus one pair across problems per problem (car 0 of problem a against car 2 of problem (7 a + 3) mod batch).  The
cars drive x = 8 t, y = -3 / 0 / 3, all perturbed, as in the tests' S cases.  Reported: pairs/s of ntg_batch_separation without a threshold
and with a required distance of 2.0 (tol = 1e-9 max sum_t S_t^2, above 64 slack), the mean of npieces and the share of pairs that end at
level 0 in both runs, and next to that the only route there is without the call for positions in the plane: the difference coefficients formed
with torch (two gathers and a subtraction) and handed to ntg_batch_extrema (sides = 1) on an obstacle-field plan with its centre at the
origin; that route has no threshold.  One JSON line at the end.
python tools/separation_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extrema_oracle as xo        # the tests' Greville abscissae
import separation_oracle as po     # ... and slack
from ntg_amd import api, configs as cf

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
SEP = 2.0
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


spec = cf.config_M()
gv = xo.greville(spec)
n = gv.size
rng = np.random.default_rng(86)
xh = np.concatenate([v for c in range(3) for v in (8.0 * gv + rng.standard_normal((batch, n)), 3.0 * (c - 1) + rng.standard_normal((batch, n)))], axis=1)
bodies = np.array([[0, 1], [2, 3], [4, 5]], dtype=np.int32)
ph = np.array([p for a in range(batch) for p in ((a, a, 0, 1), (a, a, 0, 2), (a, a, 1, 2), (a, (7 * a + 3) % batch, 0, 2))], dtype=np.int32)
npairs = len(ph)
S2 = float(po.slack(spec, xh, bodies, ph, 0).max()) * 2.0 ** 39
tol = 1e-9 * S2

plan = api.Plan(spec, 0)
x = torch.from_numpy(xh).to("cuda:0")
pairs = torch.from_numpy(ph).to("cuda:0")
sep = torch.full((npairs,), SEP, dtype=torch.float64, device="cuda:0")
mn = torch.empty((npairs, 2), dtype=torch.float64, device="cuda:0"); viol = torch.empty_like(mn)
status = torch.empty(npairs, dtype=torch.int32, device="cuda:0"); npieces = torch.empty_like(status)
st = plan._stream()


def call_sep(thr):   # the C entry point on preallocated outputs: the allocation is not the kernel's
    rc = L.ntg_batch_separation(plan.h, batch, x.data_ptr(), 3, 2, bodies.ctypes.data_as(api.ip), 0, npairs, pairs.data_ptr(), sep.data_ptr() if thr else None, tol, 30,
                                mn.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), viol.data_ptr() if thr else None, st)
    assert rc == 0, L.ntg_last_error().decode()


res = dict(tool="separation_rate", batch=batch, npairs=npairs, tol=tol)
for thr in (False, True):
    ms = rate(lambda: call_sep(thr))
    torch.cuda.synchronize()
    s, k = status.cpu().numpy(), npieces.cpu().numpy()
    key = "sep%g" % SEP if thr else "nosep"
    res[key] = dict(ms=round(ms, 4), pairs_per_s=round(npairs / ms * 1e3), npieces_mean=round(float(k.mean()), 1), level0=float((k == 20).mean()), status_ok=float((s == 0).mean()))
    if thr:
        v = viol.cpu().numpy()
        res[key].update(violate=float((v[:, 0] > 0).mean()), certified_clear=float((v[:, 1] == 0).mean()))
    print("ntg_batch_separation, %s: %d pairs in %.4f ms = %.3g pairs/s; %.1f polygons per pair, %.3f of the pairs end at level 0, status OK %.3f"
          % ("required distance %g" % SEP if thr else "no threshold", npairs, ms, npairs / ms * 1e3, res[key]["npieces_mean"], res[key]["level0"], res[key]["status_ok"]))
call_sep(False); torch.cuda.synchronize(); ref_min = mn.cpu().numpy().copy()

# the route without the call: delta by torch, then ntg_batch_extrema on a two-output plan whose one row is x^2 + y^2
op = api.Plan(cf.config_OF(1), 0)
op.set_params(torch.zeros((npairs, 2), dtype=torch.float64, device="cuda:0"))
x3 = x.view(batch, 3, 2 * n)
ia, ib, iga, igb = (pairs[:, i].long() for i in range(4))
ext = torch.empty((npairs, 1, 4), dtype=torch.float64, device="cuda:0")
est = torch.empty((npairs, 1), dtype=torch.int32, device="cuda:0"); enp = torch.empty_like(est)
ost = op._stream()


def call_route():
    delta = x3[ia, iga] - x3[ib, igb]
    rc = L.ntg_batch_extrema(op.h, npairs, delta.data_ptr(), tol, 30, 1, None, None, ext.data_ptr(), None, est.data_ptr(), enp.data_ptr(), None, None, ost)
    assert rc == 0, L.ntg_last_error().decode()


ms = rate(call_route)
torch.cuda.synchronize()
same = bool(np.array_equal(ext.cpu().numpy()[:, 0, :2], ref_min))
res["torch_delta_extrema"] = dict(ms=round(ms, 4), pairs_per_s=round(npairs / ms * 1e3), same_bits=same)
print("torch difference + ntg_batch_extrema (sides 1) on an obstacle-field plan: %d pairs in %.4f ms = %.3g pairs/s; the same bits as ntg_batch_separation: %s"
      % (npairs, ms, npairs / ms * 1e3, same))
print(json.dumps(res))
