"""tests/bisect_oracle.py, the one level loop of the bisection calls' oracles, without a GPU.

1. Against tests/golden/oracle_levels.npz (tools/record_oracle_levels.py), recorded with the five loops it replaced -- extrema_oracle's,
   separation_oracle's, ratios_oracle's, trig_oracle's and minmax_oracle's: every stored key of every case of tests/oracle_levels_cases.py is
   equal under ==, with NaNs and signed infinities in the same places (the sign of a zero is not part of it).  One key differs by design:
   forms' margin.  The recorded one came from a tolerance object that saw only the comparisons Python's `or` evaluated; the loop now takes
   both sides of every decision, as ratios, trig and minmax always did, so it can only be smaller.  It is equal wherever a level follows the
   first (a piece that one side opened is compared again, halved, on both): everywhere but in L80, which ends FULL at level 0 (8.8e10 before,
   9.0e-9 = 549.8 slacks now), and in K4's run at max_depth = 0, which ends there too.
2. Pins between the kinds of piece, on K4's polygons: the pair, the member stack, the trig piece and separation's threshold instance each
   reduce to the single polygon."""
import os

import numpy as np
import pytest

import bisect_oracle as bo
import extrema_oracle as xo
import forms_oracle as fo
import minmax_oracle as mo
import oracle_levels_cases as lc
import ratios_oracle as ro
import separation_oracle as po
import trig_oracle as to
from ntg_amd import trig as tg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_levels.npz")
STRICTER = {"forms:L80/tol/margin", "forms:K4/d0/margin"}   # (1. above)
SAME = ("ext", "when", "status", "npieces", "depth", "max_open")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_the_cases_and_every_exit(golden):
    assert {k.split("/")[0] for k in golden} == set(lc.CASES)
    status = {(k.split(":")[0], int(s)) for k, v in golden.items() if k.endswith("/status") for s in v.reshape(-1)}
    for kind in ("forms", "trig", "minmax"):
        assert {(kind, s) for s in (xo.OK, xo.DEPTH, xo.FULL)} <= status, kind
    assert {("ratios", s) for s in (ro.OK, ro.DEPTH, ro.NAN, ro.POLE)} | {("trig", to.NAN), ("minmax", mo.NAN)} <= status
    assert golden["minmax:M16/tol/which"].max() >= 8   # (a group of 16 members decides)


@pytest.mark.parametrize("case", lc.CASES)
def test_one_loop_returns_what_the_five_returned(case, golden):
    res = lc.run_case(case)
    want = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "/")}
    assert want and set(want) <= set(res), sorted(set(want) - set(res))
    for k, w in want.items():
        g = res[k]
        assert g.shape == w.shape and g.dtype.kind == w.dtype.kind, k
        if case.startswith("forms:") and k.endswith("/margin"):
            assert (g <= w).all(), k
            if case + "/" + k in STRICTER:
                continue
        assert ((g == w) | ((g != g) & (w != w))).all(), (k, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:4].tolist())


# ---------------- 2. the kinds of piece reduce to the single polygon ----------------
@pytest.fixture(scope="module")
def k4():
    c = fo.inputs("K4")
    return c, [[xo.level_oracle(c.polys[f][b], c.kn(b, f), c.tol) for f in range(len(c.forms))] for b in range(2)]


def test_a_pair_with_a_denominator_of_ones_is_the_polygon(k4):
    c, ref = k4
    for b in range(2):
        for f in range(len(c.forms)):
            r = ro.level_oracle(c.polys[f][b], np.ones_like(c.polys[f][b]), c.kn(b, f), c.tol)
            assert all(r[k] == ref[b][f][k] for k in SAME), (b, f)
            assert r["dmin"] == 1.0


@pytest.mark.parametrize("outer, inner", [(o, i) for o in (mo.MIN, mo.MAX) for i in (mo.MIN, mo.MAX)])
def test_a_group_of_one_member_is_the_polygon(k4, outer, inner):
    c, ref = k4
    groups = [(outer, inner, [[(f, 0.0, -1)]]) for f in range(len(c.forms))]
    p0 = mo.pieces0(c.spec, c.x[:2], c.forms, groups, c.fprm[:2])
    for b in range(2):
        for f in range(len(c.forms)):
            r = mo.levels(groups[f], p0[f][b], c.kn(b, f), c.tol)
            assert all(r[k] == ref[b][f][k] for k in SAME), (b, f)
            assert r["which"] == (0, 0)


def test_a_trig_form_of_lin_terms_is_the_forms_oracle_on_that_form(k4):
    c, _ = k4
    e = lambda o, r: tg.entry(c.spec, o, r)
    pairs = [[(e(0, 0), 0.6), (e(1, 0), 0.8)], [(e(0, 1), 1.0)], [(e(1, 2), 0.25), (e(0, 0), -3.0), (e(1, 1), 2.0)]]
    tforms = [sum((tg.term(to.LIN, [u], w=w) for u, w in p), []) for p in pairs]
    qforms = [sum((fo.fm.linear(u, w) for u, w in p), []) for p in pairs]
    p0, polys = to.pieces0(c.spec, c.x[:2], tforms), fo.form_polygons(c.spec, c.x[:2], qforms)
    for b in range(2):
        for f in range(len(pairs)):
            kn = c.spec.knots[fo.shape(c.spec, qforms[f])[0]]
            r, q = to.levels(p0[f][0], p0[f][1][b], kn, c.tol), xo.level_oracle(polys[f][b], kn, c.tol)
            assert all(r[k] == q[k] for k in SAME), (b, f)


def test_separation_is_the_polygon_at_sides_1_with_the_threshold(k4):
    c, _ = k4
    went = 0
    for b in range(2):
        for f in range(len(c.forms)):
            P, kn = [[float(v) for v in B] for B in c.polys[f][b]], c.kn(b, f)
            free = po.level_sep(P, kn, c.tol)
            for s2 in (np.inf, min(min(B) for B in P)):   # (no point of the polygons lies below the second one: every piece stays shut)
                r, q = po.level_sep(P, kn, c.tol, s2), bo.levels(bo.POLYGON, P, kn, c.tol, sides=1, s2=s2)
                assert (r["min"], r["when"]) == (q["ext"][:2], q["when"][0]) and all(r[k] == q[k] for k in SAME[2:]), (b, f, s2)
                went += r["npieces"] < free["npieces"]
            q = xo.level_oracle(P, kn, c.tol, sides=1)
            assert (free["min"], free["when"]) == (q["ext"][:2], q["when"][0]) and all(free[k] == q[k] for k in SAME[2:]), (b, f)
    assert went > 0
