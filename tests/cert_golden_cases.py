"""The cases of tests/test_gpu_cert_golden.py, shared with tools/record_cert_golden.py (which records the fixture
tests/golden/cert_calls.npz): the three time certificates -- Plan.envelope, Plan.envelope_sos, Plan.extrema -- on small inputs that reach
every path of their kernels, so that a change of the code they share can be held to the recorded results bit for bit.

A case is a plan with a batch on it and a list of calls; run_case gives {"<call>/<key>": numpy array}.  A call the library refuses is
recorded too, as "<call>/error": the exception's text (the error code and the message).
  O4, O20, OF5, D8, T3, K3, G4   extrema_oracle.inputs as they stand: a partial last pass of the persistent loop (67 problems), per-problem
                                 parameters, order 8 (the KM = NTG_MAX_ORDER instance, degrees 10 and 12), a row without a statement, three
                                 linear rows one of which combines derivatives 1 and 2 (elevation), per-problem grids.  Calls: extrema at
                                 the case's tolerance, at max_depth = 0, with sides = 1 and with bounds; envelope at nsub = 0 and 2 (entries
                                 and rows, the variants of K3 below the rows alone) where the plan has linear rows -- on G4 the entries
                                 alone, the per-problem-grid kernel's -- and envelope_sos at nsub = 0 and 2 where it has nonlinear ones,
                                 both also with bounds.
  T                              config_T() unchanged, its outputs in different basis classes: envelope entries and envelope_sos at nsub = 1
  FULL80                         80 knot intervals: level 0 of the bisection forms every polygon twice, and the list overflows
  K3_nan                         problems 1 to 3 of K3, a NaN coefficient in the second of them
  K3_zero                        K3 with a fourth linear row of zeros (if ntg_plan_create refuses the plan, that is what is recorded)
"""
import dataclasses

import numpy as np
import torch

import extrema_oracle as xo
from ntg_amd import api, configs as cf
from cert_common import full_list_problem
from gpu_common import dev

CASES = xo.CASES + ["T", "FULL80", "K3_nan", "K3_zero"]
VIOL = ("viol", "where")


def zero_row_problem():
    """(spec, x, lower, upper): three problems of K3 and a fourth linear trajectory row that names nothing"""
    c = xo.inputs("K3")
    ltc = np.concatenate([np.asarray(c.spec.ltc).reshape(3, c.spec.nz), np.zeros((1, c.spec.nz))])
    spec = dataclasses.replace(c.spec, ltc=ltc, lin_ineq=[0] * c.spec.nlic + [1] * 4 + [0] * c.spec.nlfc)
    nb = 3
    lo = np.concatenate([c.lower[:nb, :9], np.full((nb, 1), -1.0), c.lower[:nb, 9:]], axis=1)
    up = np.concatenate([c.upper[:nb, :9], np.full((nb, 1), 1.0), c.upper[:nb, 9:]], axis=1)
    return spec, c.x[:nb], lo, up


def _record(res, call, fn, keep=None):
    """keep: the outputs recorded (a call with bounds returns the bounds-free call's arrays again: the fixture holds them once)"""
    try:
        out = fn()
        torch.cuda.synchronize()
        for k, v in out.items():
            if keep is None or k in keep:
                res[call + "/" + k] = v.cpu().numpy()
    except api.NtgError as e:
        res[call + "/error"] = np.array(str(e))


def _calls(res, plan, spec, x, lo, up, tol, entries=True, entries_only=False):
    xd, lod, upd = dev(x), dev(lo), dev(up)
    _record(res, "ext", lambda: plan.extrema(xd, tol))
    _record(res, "ext_d0", lambda: plan.extrema(xd, tol, max_depth=0))
    _record(res, "ext_s1", lambda: plan.extrema(xd, tol, sides=1))
    if plan.extrema_rows().all():
        _record(res, "ext_b", lambda: plan.extrema(xd, tol, lower=lod, upper=upd), VIOL)
    for nsub in (0, 2):
        if spec.nltc:
            _record(res, "env%d" % nsub, lambda: plan.envelope(xd, nsub, want_entries=entries, want_rows=True))
            _record(res, "env%d_b" % nsub, lambda: plan.envelope(xd, nsub, lower=lod, upper=upd, want_entries=False, want_rows=True), VIOL)
        elif entries_only:
            _record(res, "env%d" % nsub, lambda: plan.envelope(xd, nsub))
        if spec.nnltc:
            _record(res, "sos%d" % nsub, lambda: plan.envelope_sos(xd, nsub))
            _record(res, "sos%d_b" % nsub, lambda: plan.envelope_sos(xd, nsub, lower=lod, upper=upd), VIOL)


def run_case(name):
    """run the case on cuda:0 with the loaded library"""
    res = {}
    if name in xo.CASES or name == "K3_nan":
        c = xo.inputs("K3" if name == "K3_nan" else name)
        plan = api.Plan(c.spec, 0)
        if c.knots is not None:
            plan.set_grids(dev(c.knots), dev(c.bps), with_precond=False)
        if c.prm is not None:
            plan.set_params(dev(c.prm))
        x, lo, up = c.x, c.lower, c.upper
        if name == "K3_nan":
            x, lo, up = x[1:4].copy(), lo[1:4], up[1:4]
            x[1, 1] = np.nan   # a coefficient of x on the first knot interval: rows 1 and 2 name it, row 0 does not
        _calls(res, plan, c.spec, x, lo, up, c.tol, entries=name != "K3_nan", entries_only=name == "G4")
    elif name == "T":
        spec = cf.config_T()
        plan = api.Plan(spec, 0)
        xd = dev(np.random.default_rng(76).standard_normal((3, spec.nC)))
        _record(res, "env1", lambda: plan.envelope(xd, 1))
        _record(res, "sos1", lambda: plan.envelope_sos(xd, 1))
    elif name == "FULL80":
        spec, x = full_list_problem()
        plan = api.Plan(spec, 0)
        xd = dev(x)
        _record(res, "ext_s1", lambda: plan.extrema(xd, 0.0, sides=1))
        _record(res, "ext_d0", lambda: plan.extrema(xd, 0.0, max_depth=0))
        _record(res, "ext", lambda: plan.extrema(xd, 64 * float(xo.slack(spec, x).max())))
        _record(res, "env0", lambda: plan.envelope(xd, 0, want_entries=False, want_rows=True))
        _record(res, "sos0", lambda: plan.envelope_sos(xd, 0))
    else:
        spec, x, lo, up = zero_row_problem()
        try:
            plan = api.Plan(spec, 0)
        except api.NtgError as e:
            return {"plan/error": np.array(str(e))}
        _calls(res, plan, spec, x, lo, up, xo.inputs("K3").tol, entries=False)
    return res
