"""The oracle of ntg_batch_trig (tests/trig_oracle.py) against the truth, without a GPU: its enclosures hold the extrema of the forms sampled
densely from scipy's BSpline and polished, its attained values are the forms' values at `when`, OK means the tolerance is met, FULL and DEPTH
results stay sound and inside [-W, W], the all-LIN form is forms_oracle's, and the seeds of the GPU cases leave the decisions room."""
import numpy as np
import pytest
from scipy.interpolate import BSpline
from scipy.optimize import minimize_scalar

import envelope_oracle as eo
import extrema_oracle as xo
import forms_oracle as fo
import trig_oracle as to

NS = 200001


def _flag(c, b, ts):
    """the flat flag of problem b at the times ts: [nt, nz]"""
    spec = c.spec
    sls = eo.coef_slices(spec)
    cols = []
    for o in range(spec.nout):
        brk = spec.knots[o] if c.knots is None else c.knots[b]
        s = BSpline(eo.aug_knots(brk, spec.order[o], spec.mult[o]), c.x[b, sls[o]], spec.order[o] - 1)
        cols += [s(ts) if r == 0 else s.derivative(r)(ts) if r < spec.order[o] else np.zeros_like(ts) for r in range(spec.maxderiv[o])]
    return np.stack(cols, axis=1)


def _value(c, b, f, ts):
    ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
    fp = None if c.fprm is None else c.fprm[b:b + 1]
    return to.values(c.spec, _flag(c, b, ts)[None], [c.forms[f]], fp)[0, :, 0]


def _true_extrema(c, b, f):
    kn = np.asarray(c.kn(b, f), dtype=np.float64)
    ts = np.linspace(kn[0], kn[-1], NS)
    v = _value(c, b, f, ts)
    out = []
    for sgn in (1.0, -1.0):
        i = int(np.argmin(sgn * v))
        lo, hi = ts[max(i - 1, 0)], ts[min(i + 1, NS - 1)]
        r = minimize_scalar(lambda t: sgn * _value(c, b, f, t)[0], bounds=(lo, hi), method="bounded", options={"xatol": 1e-13})
        out.append(sgn * min(sgn * v[i], r.fun))
    return out


def _check_sound(c, b, f, r, tol):
    sl = c.sl[b, f]
    lo, hi = _true_extrema(c, b, f)
    e = r["ext"]
    assert e[0] - sl <= lo <= e[1] + sl and e[2] - sl <= hi <= e[3] + sl, (c.name, b, f, e, lo, hi)
    assert abs(_value(c, b, f, r["when"][0])[0] - e[1]) <= sl and abs(_value(c, b, f, r["when"][1])[0] - e[2]) <= sl, (c.name, b, f)
    if r["status"] == to.OK:
        assert e[1] - e[0] <= tol and e[3] - e[2] <= tol
    meta = c.p0[f][0]
    if not meta[1]:
        assert -meta[2] <= e[0] and e[3] <= meta[2]


@pytest.mark.parametrize("name", ["TA4", "TE8", "TK8", "TD", "TPP", "TMOD"])
def test_oracle_encloses_the_extrema(name):
    c = to.inputs(name)
    for tol in (to.TOL, to.TOL9):
        lv = c.levels(tol)
        for b in range(min(c.x.shape[0], 3)):
            for f in range(len(c.forms)):
                r = lv[b][f]
                assert r["status"] == to.OK and r["depth"] <= 20 and r["max_open"] <= to.CAP, (name, b, f, r["status"], r["depth"], r["max_open"])
                _check_sound(c, b, f, r, tol)


@pytest.mark.parametrize("name", to.CASES)
def test_the_seeds_leave_the_decisions_room(name):
    """at TOL every open / retire decision of the oracle keeps 16 slacks from its limit, so the device decides alike"""
    c = to.inputs(name)
    lv = c.levels(to.TOL)
    for b in range(c.x.shape[0]):
        for f in range(len(c.forms)):
            assert lv[b][f]["margin"] >= 16.0 * c.sl[b, f], (name, b, f, lv[b][f]["margin"], c.sl[b, f])


def test_full_depth_and_nan():
    c = to.inputs("TFULL")
    for b in range(c.x.shape[0]):
        r = c.levels(to.TOL9)[b][0]
        assert r["status"] == to.FULL and r["max_open"] > to.CAP
        _check_sound(c, b, 0, r, to.TOL9)
    c = to.inputs("TD")
    lv = c.levels(to.TOL9, max_depth=3)
    assert any(lv[b][f]["status"] == to.DEPTH for b in range(c.x.shape[0]) for f in range(len(c.forms)))
    for b in range(c.x.shape[0]):
        for f in range(len(c.forms)):
            _check_sound(c, b, f, lv[b][f], to.TOL9)
    c = to.inputs("TNAN")
    st = [[r["status"] for r in row] for row in c.levels(to.TOL)]
    assert st[1] == [to.NAN] * 3 and all(s == to.OK for s in st[0] + st[2])
    c = to.inputs("L80")
    assert all(r["npieces"] >= 80 for row in c.levels(to.TOL) for r in row)


def test_all_lin_forms_are_forms_oracles():
    """rule 5: ext, when, status and npieces of an all-LIN form equal forms_oracle's on the equivalent form, under =="""
    c = to.inputs("TD")
    tforms, qforms = to.lin_pin_forms(c.spec)
    p0 = to.pieces0(c.spec, c.x, tforms)
    polys = fo.form_polygons(c.spec, c.x, qforms)
    for f in range(len(tforms)):
        kn = c.spec.knots[to.shape(c.spec, tforms[f])[0]]
        for b in range(c.x.shape[0]):
            r = to.levels(p0[f][0], p0[f][1][b], kn, to.TOL9)
            q = xo.level_oracle(polys[f][b], kn, to.TOL9)
            assert tuple(r["ext"]) == tuple(q["ext"]) and tuple(r["when"]) == tuple(q["when"]) and (r["status"], r["npieces"]) == (q["status"], q["npieces"]), (f, b)
