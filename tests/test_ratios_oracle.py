"""tests/ratios_oracle.py against exact rational arithmetic, without a GPU: the float64 statement of ntg_batch_ratios's definition encloses the
true minimum and maximum of every ratio within the header's slack, meets the tolerance, keeps its decisions away from their limits (so that
the GPU tests may compare status and npieces for equality), ends every case with the status the GPU tests expect, and the header's rounding
statement covers the worst error of the float64 pairs against exact ones.  RMOD's plan needs a loaded module for the GPU only: the oracle
takes its spec as it is.
"""
from fractions import Fraction as Fr
from math import inf

import numpy as np
import pytest

import forms_oracle as fo
import ratios_oracle as ro


@pytest.fixture(scope="module", params=ro.CASES)
def case(request):
    return ro.inputs(request.param)


def test_pair_rule_on_small_polygons():
    kn = [0.0, 1.0, 3.0]
    # a denominator of ones: extrema_oracle's loop on the numerator, figure by figure
    N = [[1.0, -2.0, 0.5], [0.5, 3.0, -1.0]]
    ones = [[1.0] * 3] * 2
    a, b = ro.level_oracle(N, ones, kn, 1e-9), ro.xo.level_oracle(N, kn, 1e-9)
    for k in ("ext", "when", "status", "npieces", "depth", "max_open"):
        assert a[k] == b[k], k
    # S / S is 1.0 four times and no piece opens
    r = ro.level_oracle([[2.0, 3.0, 0.7]] * 2, [[2.0, 3.0, 0.7]] * 2, kn, 0.0)
    assert r["ext"] == (1.0, 1.0, 1.0, 1.0) and r["status"] == ro.OK and r["npieces"] == 2
    # an end with denominator <= 0: POLE after the end-taking of its level, the pairs formed so far counted
    r = ro.level_oracle([[1.0, 1.0, 1.0]] * 2, [[1.0, 1.0, 0.0], [0.0, 1.0, 1.0]], kn, 1e-9)
    assert r["status"] == ro.POLE and r["ext"] == (-inf, inf, -inf, inf) and r["npieces"] == 2 and all(np.isnan(r["when"]))
    # the denominator (t - 1/3)^2 touches zero between the ends the bisection visits: its piece stays open on every side until max_depth
    r = ro.level_oracle([[1.0, 1.0, 1.0]], [[1.0 / 9.0, -2.0 / 9.0, 4.0 / 9.0]], [0.0, 1.0], 1e-9, max_depth=6)
    assert r["status"] == ro.DEPTH and r["ext"][0] == -inf and r["ext"][3] == inf and np.isfinite(r["ext"][1:3]).all()
    # NaN before POLE
    r = ro.level_oracle([[1.0, np.nan, 1.0]], [[1.0, 1.0, 0.0]], [0.0, 1.0], 1e-9)
    assert r["status"] == ro.NAN and r["npieces"] == 1


def test_elevated_ones_stay_ones():
    """the empty side of a ratio of any degree is 1.0 bit for bit: a ratio {nnum = 1, nden = 0} divides by 1.0"""
    Q = np.ones((1, 1, 1))
    for _ in range(ro.MAXDEG):
        Q = ro.eo.elevate(Q)
        assert (Q == 1.0).all()


def test_every_case_ends_with_the_expected_status(case):
    c = case
    assert np.isfinite(c.sl).all() and (c.sl > 0).all()
    for b, row in enumerate(c.levels()):
        for r, res in enumerate(row):
            assert res["status"] == ro.OK, (c.name, b, r)
            assert res["ext"][1] - res["ext"][0] <= c.tol[r] and res["ext"][3] - res["ext"][2] <= c.tol[r]
            assert res["dmin"] > 0.0


def test_decisions_keep_their_distance(case):
    """Every comparison "plo < U - tol" / "phi > V + tol" of the float64 oracle lies at least 16 slacks of its ratio away from its limit, so
    the kernel, whose figures differ from the oracle's by less than a slack, decides every piece alike.  If a seed does not satisfy this, the
    seed changes (ratios_oracle.SEEDS), not the assertion."""
    c = case
    for b, row in enumerate(c.levels()):
        for r, res in enumerate(row):
            assert res["margin"] >= 16.0 * c.sl[b, r], (c.name, b, r, res["margin"] / c.sl[b, r])
            assert res["depth"] <= 24 and res["max_open"] <= 48, (c.name, b, r)


@pytest.mark.parametrize("name", ro.EXACT_CASES)
def test_oracle_encloses_the_exact_extrema(name):
    c = ro.inputs(name)
    lv = c.levels()
    for b in range(c.nexact):
        for r, ratio in enumerate(c.ratios):
            res, sl = lv[b][r], c.sl[b, r]
            lo, hi, vlo, vhi = (float(v) for v in ro.exact_extrema(c.spec, c.x[b], c.forms, ratio, 0.25 * sl, None if c.fprm is None else c.fprm[b], None if c.knots is None else c.knots[b]))
            e = res["ext"]
            print(f"{c.name} problem {b} ratio {r}: depth {res['depth']}, most open {res['max_open']}, min in [{e[0]:.9g}, {e[1]:.9g}] exact {lo:.9g}, "
                  f"max in [{e[2]:.9g}, {e[3]:.9g}] exact {vhi:.9g}, slack {sl:.3g}")
            assert e[0] - sl <= hi and lo <= e[1] + sl, (c.name, b, r)
            assert e[2] - sl <= vhi and vlo <= e[3] + sl, (c.name, b, r)


@pytest.mark.parametrize("name", ro.EXACT_CASES)
def test_header_rounding_statement_covers_float64_pairs(name):
    """the worst error of the float64 level-0 points against the exact ones in units of the statement's eps of their side, and of the level-0
    quotients in slacks of (eps_N + |rho| eps_D) / (d - eps_D) with the point's own d: at most 0.1 each (the halvings' share of eps, 2^-43 of
    the side, is not exercised by level 0 and is a fifteenth of the smallest eps here)"""
    c = ro.inputs(name)
    worst_pt, worst_q = 0.0, 0.0
    for b in range(c.nexact):
        for r, ratio in enumerate(c.ratios):
            ex = ro.exact_pairs(c.spec, c.x[b], c.forms, ratio, None if c.fprm is None else c.fprm[b], None if c.knots is None else c.knots[b])
            N, Q = c.pairs[r][0][b], c.pairs[r][1][b]
            eN, eD = float(ro.side_eps(c, ratio[0])[b]), float(ro.side_eps(c, ratio[1])[b])
            for j in range(N.shape[0]):
                for s in range(N.shape[1]):
                    en, ed = abs(Fr(float(N[j, s])) - ex[j][0][s]), abs(Fr(float(Q[j, s])) - ex[j][1][s])
                    worst_pt = max(worst_pt, float(en) / eN, float(ed) / eD)
                    if Q[j, s] > eD and ex[j][1][s] > 0:
                        rho = ex[j][0][s] / ex[j][1][s]
                        err = abs(Fr(float(N[j, s] / Q[j, s])) - rho)
                        worst_q = max(worst_q, float(err) / ((eN + abs(float(rho)) * eD) / (float(Q[j, s]) - eD)))
    print(f"{c.name}: float64 points differ from the exact ones by at most {worst_pt:.3g} eps of their side, quotients by at most {worst_q:.3g} slack")
    assert worst_pt <= 0.1 and worst_q <= 0.1


def test_every_case_at_the_fine_tolerance(case):
    """at 1e-9 of every ratio's largest quotient every case ends OK within the tolerance, at least 18 levels deep; kappa^2 on 20 knot intervals
    keeps 40 or more pairs open at once, under the cap of 64.  The decisions' margins are far below the slack here (printed): the GPU test
    asserts that the kernel decides alike, the rounding statement does not imply it"""
    c = case
    lv = c.levels(c.fine)
    most, deep = max(res["max_open"] for row in lv for res in row), max(res["depth"] for row in lv for res in row)
    margin = min(res["margin"] / c.sl[b, r] for b, row in enumerate(lv) for r, res in enumerate(row))
    print(f"{c.name} at 1e-9: most open {most}, depth {deep}, pairs per ratio up to {max(res['npieces'] for row in lv for res in row)}, smallest margin {margin:.3g} slack")
    for row in lv:
        for r, res in enumerate(row):
            assert res["status"] == ro.OK and res["ext"][1] - res["ext"][0] <= c.fine[r] and res["ext"][3] - res["ext"][2] <= c.fine[r]
    assert deep >= 18 and most <= ro.xo.CAP
    if c.name == "RK20":
        assert most >= 40


def test_tight_certificate_beats_the_loose_bound():
    """steering: L sqrt(max_hi of kappa^2) <= steering_bound of the two forms, on every problem of RK20"""
    c = ro.inputs("RK20")
    k2 = np.array([row[0]["ext"][3] for row in c.levels()])
    f = fo.Inputs("f", c.spec, c.x, c.forms[:2])
    f.sl, f.polys = c.fsl[:, :2], c.fpolys[:2]
    ext = np.array([[res["ext"] for res in row] for row in f.levels(float(c.tol[0]))])
    loose = fo.fm.steering_bound(ext, 3.0)
    tight = 3.0 * np.sqrt(k2)
    print("RK20: loose / tight steering bound", np.round(loose / tight, 2))
    assert (tight <= loose * (1.0 + 1e-9)).all()
