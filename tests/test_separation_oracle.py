"""tests/separation_oracle.py on the very inputs the GPU tests use, without a GPU: without a threshold its level function is
extrema_oracle.level_oracle at sides = 1, bit for bit; it encloses the exact minimum (rational bisection) to the slack; and with and without
the threshold it ends every pair with status OK at depth <= 24 with at most 32 open pieces at any level.  Those margins to the limits of 30
and 64 are a condition on the inputs, not a measurement: rounding differences on the device cannot tip a pair into DEPTH or FULL, so the GPU
tests may leave out no pair."""
import numpy as np
import pytest

import extrema_oracle as xo
import separation_oracle as po

IDS = [f"{n}-d{d}" for n, d in po.CASES]


@pytest.fixture(scope="module", params=po.CASES, ids=IDS)
def case(request):
    return po.inputs(*request.param)


def test_without_a_threshold_the_levels_are_the_extrema_oracle_at_sides_1(case):
    for P, got in zip(case.polys, case.levels()):
        ref = xo.level_oracle(P, case.kn(), case.tol, sides=1)
        assert got["min"] == ref["ext"][:2] and got["when"] == ref["when"][0] and got["npieces"] == ref["npieces"] and got["status"] == ref["status"]


def test_the_exact_minimum_is_enclosed(case):
    worst = 0.0
    for q in range(3):
        s = case.sl[q]
        elo, ehi = po.exact_min(case.spec, case.dl[q], int(case.bodies[0, 0]), case.deriv, s / 8)
        assert ehi - elo <= s / 8
        for s2 in (np.inf, case.sep ** 2):
            mlo, mhi = case.levels(s2)[q]["min"]
            worst = max(worst, (mlo - ehi) / s, (elo - mhi) / s)
            assert mlo >= min(mhi - case.tol, s2)
    print(f"{case.name} deriv {case.deriv}: the exact minimum outside the enclosures by at most {worst:.3g} slack")
    assert worst <= 1.0


def test_inputs_keep_their_distance_from_the_limits(case):
    depth = nopen = 0
    for s2 in (np.inf, case.sep ** 2):
        for got in case.levels(s2):
            assert got["status"] == po.OK
            depth, nopen = max(depth, got["depth"]), max(nopen, got["max_open"])
    thr = case.levels(case.sep ** 2)
    viol = sum(po.violation(g["min"], case.sep ** 2)[0] > 0 for g in thr)
    print(f"{case.name} deriv {case.deriv}: tol {case.tol:.3g}, deepest level {depth}, most open pieces {nopen}; with sep {case.sep}: "
          f"{sum(g['depth'] == 0 for g in thr)} of {len(thr)} pairs end at level 0, {viol} violate")
    assert depth <= 24 and nopen <= 32


def test_s4_is_the_case_the_issue_describes():
    c = po.inputs("S4")
    assert c.pairs.shape == (201, 4) and sum(a == b and ga == gb for a, b, ga, gb in c.pairs) == 1
    zero = [q for q, (a, b, ga, gb) in enumerate(c.pairs) if a == b and ga == gb][0]
    assert not c.polys[zero].any() and c.levels()[zero]["min"] == (0.0, 0.0)
    thr = c.levels(c.sep ** 2)
    at0 = [g for g in thr if g["depth"] == 0]
    assert len(at0) == 85 and all(g["npieces"] == 4 for g in at0)
    assert sum(po.violation(g["min"], c.sep ** 2)[0] > 0 for g in thr) == 110
