"""The oracle of ntg_batch_minmax (tests/minmax_oracle.py) against the truth, without a GPU: its enclosures hold the extrema of the groups
sampled densely from scipy's BSpline and polished on both sides of the best sample (an extremum at a kink is no stationary point), its
attained values are the groups' values at `when`, `which` names a member that attains them, OK means the tolerance is met, the kink cases
reach 1e-6 within depth 24 and those chosen for 1e-9 within depth 30, FULL, DEPTH and NAN results are what they should be, the single-member
group is forms_oracle's, and the seeds of the GPU cases leave the decisions and the `which` ties room."""
import numpy as np
import pytest
from scipy.interpolate import BSpline

import envelope_oracle as eo
import extrema_oracle as xo
import forms_oracle as fo
import minmax_oracle as mo

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


def _members(c, b, g, ts):
    ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
    fp = None if c.fprm is None else c.fprm[b:b + 1]
    return mo.member_values(c.spec, _flag(c, b, ts)[None], c.forms, c.groups[g], fp)[0]


def _value(c, b, g, ts):
    return mo.fold(c.groups[g], _members(c, b, g, ts))


def _golden(f, lo, hi):
    """the smallest value a golden-section search sees on [lo, hi], run down to the resolution of the times: at a kink the value errs by
    slope * dt, and Brent's sqrt(eps) floor on dt (scipy's bounded minimiser) would leave 1e-7 there"""
    q = 0.5 * (5.0 ** 0.5 - 1.0)
    a, b = lo, hi
    x1, x2 = b - q * (b - a), a + q * (b - a)
    f1, f2 = f(x1), f(x2)
    best = min(f(a), f(b), f1, f2)
    for _ in range(90):
        if f1 < f2:
            b, x2, f2 = x2, x1, f1
            x1 = b - q * (b - a)
            f1 = f(x1)
        else:
            a, x1, f1 = x1, x2, f2
            x2 = a + q * (b - a)
            f2 = f(x2)
        best = min(best, f1, f2)
    return best


def _true_extrema(c, b, g):
    kn = np.asarray(c.kn(b, g), dtype=np.float64)
    ts = np.linspace(kn[0], kn[-1], NS)
    v = _value(c, b, g, ts)
    out = []
    for sgn in (1.0, -1.0):
        i = int(np.argmin(sgn * v))
        best = sgn * v[i]
        for lo, hi in ((ts[max(i - 1, 0)], ts[i]), (ts[i], ts[min(i + 1, NS - 1)])):   # both sides of the best sample: a kink has two slopes
            if hi > lo:
                best = min(best, _golden(lambda t: sgn * _value(c, b, g, t)[0], lo, hi))
        out.append(sgn * best)
    return out


def _check_sound(c, b, g, r, tol):
    sl = c.sl[b, g]
    lo, hi = _true_extrema(c, b, g)
    e = r["ext"]
    assert e[0] - sl <= lo <= e[1] + sl and e[2] - sl <= hi <= e[3] + sl, (c.name, b, g, e, lo, hi)
    for s in range(2):
        mv = _members(c, b, g, r["when"][s])[0]
        assert abs(mo.fold(c.groups[g], mv) - e[1 + s]) <= sl, (c.name, b, g, s)
        assert 0 <= r["which"][s] < mv.size and abs(mv[r["which"][s]] - e[1 + s]) <= sl, (c.name, b, g, s, r["which"])
    if r["status"] == mo.OK:
        assert e[1] - e[0] <= tol and e[3] - e[2] <= tol


@pytest.mark.parametrize("name", mo.CASES)
def test_oracle_encloses_the_extrema(name):
    c = mo.inputs(name)
    for tol, depth in ((mo.TOL, 24), (mo.TOL9, 30)):
        if tol == mo.TOL9 and name not in mo.CASES9:
            continue
        lv = c.levels(tol)
        for b in range(min(c.x.shape[0], 3)):
            for g in range(len(c.groups)):
                r = lv[b][g]
                assert r["status"] == mo.OK and r["depth"] <= depth and r["max_open"] <= mo.CAP, (name, tol, b, g, r["status"], r["depth"], r["max_open"])
                _check_sound(c, b, g, r, tol)


@pytest.mark.parametrize("name", mo.CASES)
def test_the_kinks_close_and_the_seeds_leave_the_decisions_room(name):
    """every problem of every GPU case: OK at 1e-6 within depth 24 (1e-9 within depth 30 where chosen for it); at 1e-6 every open / retire
    decision of the oracle keeps 16 slacks from its limit and so does every tie that `which` rests on, so the device decides alike"""
    c = mo.inputs(name)
    lv = c.levels(mo.TOL)
    for b in range(c.x.shape[0]):
        for g in range(len(c.groups)):
            r = lv[b][g]
            assert r["status"] == c.expect and r["depth"] <= 24, (name, b, g, r["status"], r["depth"])
            assert r["margin"] >= 16.0 * c.sl[b, g], (name, b, g, r["margin"], c.sl[b, g])
            assert r["tie"] >= 16.0 * c.sl[b, g], (name, b, g, r["tie"], c.sl[b, g])
    if name in mo.CASES9:
        assert all(r["status"] == mo.OK and r["depth"] <= 30 for row in c.levels(mo.TOL9) for r in row)


def test_a_kink_is_where_the_minimum_of_a_max_group_sits():
    """MQ8, MAX of a disc and a half plane: in some problem the minimum is attained where the two cross -- the deciding member changes
    across `when` -- and the enclosure there needs more levels than any smooth extremum of the case"""
    c = mo.inputs("MQ8")
    lv = c.levels(mo.TOL)
    kinks = 0
    for b in range(c.x.shape[0]):
        t = lv[b][0]["when"][0]
        mv = _members(c, b, 0, [t - 1e-4, t + 1e-4])
        kinks += int(np.argmax(mv[0]) != np.argmax(mv[1]))
    assert kinks > 0


def test_full_depth_and_nan():
    c = mo.inputs("MFULL")
    for b in range(c.x.shape[0]):
        r = c.levels(mo.TOL9)[b][0]
        assert r["status"] == mo.FULL and r["max_open"] > mo.CAP
        _check_sound(c, b, 0, r, mo.TOL9)
    c = mo.inputs("MQ8")
    lv = c.levels(mo.TOL9, max_depth=3)
    assert any(lv[b][0]["status"] == mo.DEPTH for b in range(c.x.shape[0]))
    for b in range(3):
        _check_sound(c, b, 0, lv[b][0], mo.TOL9)
    c = mo.inputs("MNAN")
    lv = c.levels(mo.TOL)
    st = [[r["status"] for r in row] for row in lv]
    assert st[1] == [mo.NAN] * 4 and all(s == mo.OK for s in st[0] + st[2])
    assert all(r["which"] == (-1, -1) and np.isnan(r["ext"]).all() for r in lv[1])
    c = mo.inputs("ML80")
    assert all(r["npieces"] > 80 for row in c.levels(mo.TOL) for r in row)


def test_single_member_groups_are_forms_oracles():
    """pin 1: ext, when, status and npieces of a group of one member with c = 0.0 and pc = -1 equal forms_oracle's on that form, under ==;
    pin 2: repeating the member changes nothing; pin 3: the negated declaration returns the negated figures with the sides exchanged"""
    c = mo.inputs("MK8")
    polys = fo.form_polygons(c.spec, c.x, c.forms)
    for f in (0, len(c.forms) - 1):   # a face (degree 7) and a disc (degree 14)
        kn = c.spec.knots[fo.shape(c.spec, c.forms[f])[0]]
        twice = [(mo.MIN, mo.MAX, [[(f, 0.0, -1)], [(f, 0.0, -1)]]), (mo.MAX, mo.MIN, [[(f, 0.0, -1), (f, 0.0, -1)]])]
        p1 = mo.pieces0(c.spec, c.x, c.forms, [mo.single_member(f)] + twice)
        for b in range(c.x.shape[0]):
            q = xo.level_oracle(polys[f][b], kn, mo.TOL9)
            for g, grp in enumerate([mo.single_member(f)] + twice):
                r = mo.levels(grp, p1[g][b], kn, mo.TOL9)
                assert tuple(r["ext"]) == tuple(q["ext"]) and tuple(r["when"]) == tuple(q["when"]) and (r["status"], r["npieces"]) == (q["status"], q["npieces"]), (f, b, g)
                assert r["which"] == (0, 0)
    c = mo.inputs("MP4")
    nf, ng, nfp = mo.negated(c.forms, c.groups, c.fprm)
    pn = mo.pieces0(c.spec, c.x, nf, ng, nfp)
    for b in range(4):
        for g in range(len(c.groups)):
            r, n = c.levels(mo.TOL)[b][g], mo.levels(ng[g], pn[g][b], c.kn(b, g), mo.TOL)
            assert tuple(n["ext"]) == (-r["ext"][3], -r["ext"][2], -r["ext"][1], -r["ext"][0]) and tuple(n["when"]) == r["when"][::-1], (b, g)
            assert n["which"] == r["which"][::-1] and (n["status"], n["npieces"]) == (r["status"], r["npieces"]), (b, g)
