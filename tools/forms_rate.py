"""Diagnostic (not a test): ntg_batch_forms on the shapes of the tests' cases at a batch of a few thousand.  Reported per case: forms/s, the
mean of npieces per form (polygons per form) and the share of forms that end with status OK, at the case's own tolerance
(max(1e-9 max |polygon point|, 64 slack), taken from the first 64 problems).

  K4 / K20  kincar, order 6, 4 / 20 knot intervals: six forms (speed^2, the turning numerator, v . a, a half plane, an ellipse, x^2 + x' y'')
            / two (speed^2, the turning numerator).  Cars drive x = 8 t, y = 0.5, both perturbed, as in the tests.
  D8        the quadrotor, order 8, 8 intervals (the KM = 10 instances): weighted thrust, x' y''' - y' x'''.
  PP        K4's first two forms on per-problem grids (scales 0.5 .. 2).
K4's speed^2 is also timed alone: what one certificate costs next to six.  One JSON line at the end.
python tools/forms_rate.py [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forms_oracle as fo          # the tests' forms, coefficients and slack
from cert_common import scaled_grids
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


def inputs(name):
    """(spec, x [batch, nC], forms, fprm or None, knots, bps)"""
    if name == "D8":
        c = fo.inputs("D8")
        return c.spec, np.random.default_rng(195).standard_normal((batch, c.spec.nC)), c.forms, None, None, None
    l = 20 if name == "K20" else 4
    spec = cf._kincar_spec(1, 6, 3, l, 5 * l + 1, 5.0, f"kincar-2out-k6-l{l}")
    x = fo.kincar_x(spec, batch, 191, *((0.1, 0.3) if name == "K20" else ()))
    forms, fprm, knots, bps = fo.kincar_forms(spec, name == "K4"), None, None, None
    if name == "K4":
        rng = np.random.default_rng(192)
        fprm = np.stack([rng.uniform(-1.0, 1.0, batch), rng.uniform(10.0, 30.0, batch), rng.uniform(-2.0, 2.0, batch)], axis=1)
    if name == "PP":
        scales = np.linspace(0.5, 2.0, batch)
        knots, bps = scaled_grids(spec, scales)
        x[:, :spec.ncoef[0]] *= scales[:, None]
    return spec, x, forms, fprm, knots, bps


res = dict(tool="forms_rate", batch=batch)
for name in ("K4", "K20", "D8", "PP"):
    spec, xh, forms, fh, knots, bps = inputs(name)
    nform = len(forms)
    head = slice(0, 64)
    sl = fo.slack(spec, xh[head], forms, None if fh is None else fh[head], None if knots is None else knots[head])
    polys = fo.form_polygons(spec, xh[head], forms, None if fh is None else fh[head], None if knots is None else knots[head])
    tol = max(1e-9 * max(float(np.abs(P).max()) for P in polys), 64.0 * float(sl.max()))
    plan = api.Plan(spec, 0)
    if knots is not None:
        plan.set_grids(torch.from_numpy(knots).to("cuda:0"), torch.from_numpy(bps).to("cuda:0"))
    x = torch.from_numpy(xh).to("cuda:0")
    fprm = None if fh is None else torch.from_numpy(fh).to("cuda:0")
    ext = torch.empty((batch, nform, 4), dtype=torch.float64, device="cuda:0")
    status = torch.empty((batch, nform), dtype=torch.int32, device="cuda:0"); npieces = torch.empty_like(status)
    st = plan._stream()

    def call(fs=forms):   # the C entry point on preallocated outputs: the allocation is not the kernel's
        nt = (api.C.c_int * len(fs))(*[len(f) for f in fs])
        flat = [api.FormTerm(*t) for f in fs for t in f]
        rc = L.ntg_batch_forms(plan.h, batch, x.data_ptr(), len(fs), nt, (api.FormTerm * len(flat))(*flat), 0 if fprm is None else fprm.shape[1],
                               None if fprm is None else fprm.data_ptr(), tol, 30, 3, None, None, ext.data_ptr(), None, status.data_ptr(), npieces.data_ptr(), None, None, st)
        assert rc == 0, L.ntg_last_error().decode()

    ms = rate(call)
    torch.cuda.synchronize()
    s, k = status.cpu().numpy(), npieces.cpu().numpy()
    res[name] = dict(nform=nform, tol=tol, ms=round(ms, 4), forms_per_s=round(batch * nform / ms * 1e3), npieces_mean=round(float(k.mean()), 1), status_ok=float((s == 0).mean()))
    print("ntg_batch_forms, %s: %d problems x %d forms in %.4f ms = %.3g forms/s; %.1f polygons per form, status OK %.3f"
          % (name, batch, nform, ms, batch * nform / ms * 1e3, res[name]["npieces_mean"], res[name]["status_ok"]))
    if name == "K4":
        ms1 = rate(lambda: call(forms[:1]))
        res["K4_speed2_alone"] = dict(ms=round(ms1, 4), forms_per_s=round(batch / ms1 * 1e3))
        print("ntg_batch_forms, K4, speed^2 alone: %d forms in %.4f ms = %.3g forms/s" % (batch, ms1, batch / ms1 * 1e3))
print(json.dumps(res))
