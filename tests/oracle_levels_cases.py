"""The cases of tests/test_oracle_levels_golden.py, shared with tools/record_oracle_levels.py (which records the fixture
tests/golden/oracle_levels.npz): what the five oracles of the bisection calls return on their own seeded inputs, so that a change of the
level loop they share (tests/bisect_oracle.py) can be held to the recorded results under ==.  Only results are stored.

A case is "<oracle>:<inputs>"; run_case gives {"<run>/<key>": numpy array over the (problem, row) results of the run, problems first}.
Every run takes every problem of the case, at the case's own tolerance unless its name says otherwise.
  extrema:O4 .. G4        extrema_oracle.CASES, every flagged row.
  forms:K4 .. PP          forms_oracle's cases but MOD, through decision_margin.  L80 overflows the list at level 0: FULL.  K4 also at
                          sides = 1, sides = 2 and max_depth = 0.
  sep:S4-d0 .. Q8-d1      separation_oracle.CASES, without and with the required distance (thr).
  ratios:RK4 .. R8        ratios_oracle's cases but RMOD, at tol and at fine.  RK4 also at max_depth = 3 (DEPTH), with problem 7 parked (POLE)
                          and with the NaN coefficient (NAN).
  trig:TA4 .. TNAN        trig_oracle.CASES but TMOD, and TFULL (FULL) and TNAN (NAN); TD also at 1e-9 and max_depth = 3 (DEPTH).
  minmax:MP4 .. MNAN      minmax_oracle.CASES but MMOD (M16: a group of 16 members), and MFULL (FULL) and MNAN (NAN); MQ8 also at 1e-9 and
                          max_depth = 3 (DEPTH).
The cases that need a built module are left out: they run nothing of the loop that these do not."""
import numpy as np

import extrema_oracle as xo
import forms_oracle as fo
import minmax_oracle as mo
import ratios_oracle as ro
import separation_oracle as po
import trig_oracle as to

CASES = (["extrema:" + n for n in xo.CASES] + ["forms:" + n for n in fo.EXACT_CASES] + ["sep:%s-d%d" % nd for nd in po.CASES]
         + ["ratios:" + n for n in ro.EXACT_CASES] + ["trig:" + n for n in to.CASES if n != "TMOD"] + ["trig:TFULL", "trig:TNAN"]
         + ["minmax:" + n for n in mo.CASES if n != "MMOD"] + ["minmax:MFULL", "minmax:MNAN"])


def _extrema(name):
    c = xo.inputs(name)
    rows = [(r, o0) for r, (flag, o0, *_) in enumerate(xo.row_table(c.spec)) if flag]
    return {"tol": [xo.level_oracle(c.polys[r][b], c.kn(b, o0), c.tol) for b in range(c.x.shape[0]) for r, o0 in rows]}


def _forms(name):
    c = fo.inputs(name)

    def run(**kw):
        out = []
        for b in range(c.x.shape[0]):
            for f in range(len(c.forms)):
                margin, r = fo.decision_margin(c.polys[f][b], c.kn(b, f), c.tol, **kw)
                out.append(dict(r, margin=margin))
        return out

    res = {"tol": run()}
    if name == "K4":
        res.update(s1=run(sides=1), s2=run(sides=2), d0=run(max_depth=0))
    return res


def _sep(name):
    c = po.inputs(name[:-3], int(name[-1]))
    return {"tol": c.levels(), "thr": c.levels(c.sep ** 2)}


def _ratios(name):
    c = ro.inputs(name)
    flat = lambda lv: [r for row in lv for r in row]
    res = {"tol": flat(c.levels()), "fine": flat(c.levels(c.fine))}
    if name == "RK4":
        res["d3"] = flat(c.levels(max_depth=3))
        park = ro.pair_polygons(c.spec, ro.parked_x(c), c.forms, c.ratios, c.fprm, c.knots)
        res["park"] = [ro.level_oracle(N[b], Q[b], c.kn(b, r), c.tol[r]) for b in range(c.x.shape[0]) for r, (N, Q) in enumerate(park)]
        bad = ro.pair_polygons(c.spec, ro.nan_x(c), c.forms, ro.NAN_RATIOS, c.fprm, c.knots)
        res["nan"] = [ro.level_oracle(N[b], Q[b], c.kn(b, 0), c.tol[0]) for b in range(c.x.shape[0]) for N, Q in bad]
    return res


def _stacks(mod, name, deep):
    """trig_oracle and minmax_oracle alike: at TOL, and the case `deep` at TOL9 and max_depth = 3"""
    c = mod.inputs(name)
    flat = lambda lv: [r for row in lv for r in row]
    res = {"tol": flat(c.levels(mod.TOL))}
    if name == deep:
        res["d3"] = flat(c.levels(mod.TOL9, max_depth=3))
    return res


def run_case(case):
    kind, name = case.split(":")
    runs = {"extrema": _extrema, "forms": _forms, "sep": _sep, "ratios": _ratios, "trig": lambda n: _stacks(to, n, "TD"), "minmax": lambda n: _stacks(mo, n, "MQ8")}[kind](name)
    return {run + "/" + k: np.array([r[k] for r in res]) for run, res in runs.items() for k in res[0]}
