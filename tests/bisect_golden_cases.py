"""The cases of tests/test_gpu_bisect_golden.py, shared with tools/record_cert_golden.py (which records the fixture
tests/golden/bisect_calls.npz): the three bisection calls that tests/cert_golden_cases.py does not cover -- Plan.separation, Plan.forms,
Plan.ratios -- on the inputs their oracles define, so that a change of the level loop they share with Plan.extrema can be held to the
recorded results bit for bit.  Only outputs are stored.

A case is a plan with a batch on it and a list of calls; run_case gives {"<call>/<key>": numpy array}, a refusal as "<call>/error".
  S4-d0, S20-d0, Q8-d0, Q8-d1   separation_oracle.CASES.  sep: at the case's tolerance; sep_thr: with the required distance (the threshold
                                instance of the level loop); sep_d0: max_depth = 0; sep_bad: three good pairs between three with an index
                                one past an end (problem -1, problem batch, body nbody), with the required distance.
  K4, K20, L80, D8, T4, PP      forms_oracle's cases but MOD.  forms: at the case's tolerance; forms_s1: sides = 1; forms_b: with bounds
                                (the medians of the oracle's attained extrema, the last form unbounded; viol and where alone are kept);
                                forms_d0: max_depth = 0.  L80: 80 intervals, two rounds of level 0 and a list that overflows there; D8: the
                                KM = NTG_MAX_ORDER instance; T4: two basis classes; PP: per-problem grids.
  RK4, RK20, RPP, R8            ratios_oracle's cases but RMOD.  r<i> / r<i>_fine: ratio i in a call of its own at the case's tolerance /
                                at 1e-9 of its largest quotient, with bounds (the medians of the oracle's attained extrema).  RK4 also:
                                r<i>_d3 (max_depth = 3), r<i>_park (problem 7 stands still on knot interval 1: a pole where the ratio has
                                a denominator) and nan (a NaN coefficient of y in problem 5, four ratios of which two name y).
  RK100                         five problems on 100 knot intervals: workgroups of two waves, every pair formed twice; r0 ends OK past
                                level 0, r0_fine overflows the list at level 0.
MOD and RMOD need a built module and run no other device code: they are left out.
Every case goes past level 0 at its working tolerance (some npieces exceeds the number of knot intervals) with one exception that is the
case's purpose: L80's forms open all 80 intervals at level 0, the list overflows there, and every form ends FULL with npieces == 80."""
import numpy as np
import torch

import forms_oracle as fo
import ratios_oracle as ro
import separation_oracle as po
from cert_golden_cases import VIOL, _record
from gpu_common import dev
from ntg_amd import api, configs as cf, forms as fm

MAX_ORDER = 10   # NTG_MAX_ORDER
SEP_CASES = ["%s-d%d" % nd for nd in po.CASES]
FORM_CASES = [c for c in fo.CASES if c != "MOD"]
RATIO_CASES = [c for c in ro.CASES if c != "RMOD"]
CASES = SEP_CASES + FORM_CASES + RATIO_CASES + ["RK100"]
NAN_RATIOS = ro.NAN_RATIOS


def rk100():
    """tests/test_gpu_ratios.py's five problems on 100 knot intervals"""
    spec = cf._kincar_spec(1, 6, 3, 100, 501, 5.0, "kincar-2out-k6-l100")
    forms, kappa2 = fm.curvature2(spec, (0, 1))
    return ro.Inputs("RK100", spec, fo.kincar_x(spec, 5, 13, 0.002, 0.006), forms, [kappa2]).finish()


def ratio_inputs(name):
    return rk100() if name == "RK100" else ro.inputs(name)


def ratio_instance(spec, forms, ratios):
    """(KM, KR) of the kernel instance a call with these ratios runs: the forms' polygons hold the plan's largest order, the pairs' the
    call's largest degree"""
    dmax = max(max(ro.ratio_shape(spec, forms, r)[1:]) for r in ratios)
    small = max(spec.order) <= 6
    return (6 if small else MAX_ORDER, 13 if small and dmax <= 12 else 25)


def median_bounds(ext, nb, open_last=False):
    """bounds that cut through the ranges: the medians over the batch of the oracle's attained minimum and maximum, for every problem"""
    ext = np.array([[r["ext"] for r in row] for row in ext])
    lo, up = np.tile(np.median(ext[:, :, 1], axis=0), (nb, 1)), np.tile(np.median(ext[:, :, 2], axis=0), (nb, 1))
    if open_last:
        lo[:, -1], up[:, -1] = -cf.INF_BOUND, cf.INF_BOUND
    return lo, up


def bad_pairs(c):
    nb, nbody = c.x.shape[0], len(c.bodies)
    return np.array([c.pairs[0], (-1, 0, 0, 0), c.pairs[1], (0, nb, 0, 0), c.pairs[2], (0, 0, nbody, 0)], dtype=np.int32)


def _separation(res, name):
    c = po.inputs(name[:-3], int(name[-1]))
    plan, xd, pd = api.Plan(c.spec, 0), dev(c.x), dev(c.pairs, torch.int32)
    sd = dev(np.full(len(c.pairs), c.sep))
    _record(res, "sep", lambda: plan.separation(xd, pd, c.bodies, c.deriv, tol=c.tol))
    _record(res, "sep_thr", lambda: plan.separation(xd, pd, c.bodies, c.deriv, tol=c.tol, sep=sd))
    _record(res, "sep_d0", lambda: plan.separation(xd, pd, c.bodies, c.deriv, tol=c.tol, max_depth=0))
    _record(res, "sep_bad", lambda: plan.separation(xd, dev(bad_pairs(c), torch.int32), c.bodies, c.deriv, tol=c.tol, sep=sd[:6].contiguous()))


def _forms(res, name):
    c = fo.inputs(name)
    plan = api.Plan(c.spec, 0)
    if c.knots is not None:
        plan.set_grids(dev(c.knots), dev(c.bps))
    xd, fd = dev(c.x), None if c.fprm is None else dev(c.fprm)
    lo, up = median_bounds(c.levels(), c.x.shape[0], open_last=True)
    _record(res, "forms", lambda: plan.forms(xd, c.forms, c.tol, fprm=fd))
    _record(res, "forms_s1", lambda: plan.forms(xd, c.forms, c.tol, sides=1, fprm=fd))
    _record(res, "forms_b", lambda: plan.forms(xd, c.forms, c.tol, fprm=fd, lower=dev(lo), upper=dev(up)), VIOL)
    _record(res, "forms_d0", lambda: plan.forms(xd, c.forms, c.tol, max_depth=0, fprm=fd))


def _ratios(res, name):
    c = ratio_inputs(name)
    plan = api.Plan(c.spec, 0)
    if c.knots is not None:
        plan.set_grids(dev(c.knots), dev(c.bps))
    xd = dev(c.x)
    if name == "RK100":
        _record(res, "r0", lambda: plan.ratios(xd, c.forms, c.ratios, float(c.tol[0])))
        _record(res, "r0_fine", lambda: plan.ratios(xd, c.forms, c.ratios, float(c.fine[0])))
        return
    lo, up = median_bounds(c.levels(), c.x.shape[0])
    for r, ratio in enumerate(c.ratios):
        kw = dict(lower=dev(lo[:, r:r + 1]), upper=dev(up[:, r:r + 1]))
        _record(res, "r%d" % r, lambda: plan.ratios(xd, c.forms, [ratio], float(c.tol[r]), **kw))
        _record(res, "r%d_fine" % r, lambda: plan.ratios(xd, c.forms, [ratio], float(c.fine[r]), **kw))
        if name == "RK4":
            _record(res, "r%d_d3" % r, lambda: plan.ratios(xd, c.forms, [ratio], float(c.tol[r]), 3))
            _record(res, "r%d_park" % r, lambda: plan.ratios(dev(ro.parked_x(c)), c.forms, [ratio], float(c.tol[r]), **kw))
    if name == "RK4":
        _record(res, "nan", lambda: plan.ratios(dev(ro.nan_x(c)), c.forms, ro.NAN_RATIOS, float(c.tol[0])))


def run_case(name):
    """run the case on cuda:0 with the loaded library"""
    res = {}
    (_separation if name in SEP_CASES else _forms if name in FORM_CASES else _ratios)(res, name)
    return res
