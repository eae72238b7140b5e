"""tests/forms_oracle.py against exact rational arithmetic, without a GPU: the float64 statement of ntg_batch_forms's definition encloses the
true minimum and maximum of every form within the header's slack, meets the tolerance, keeps its decisions away from their limits (so that
the GPU tests may compare status and npieces for equality), and the header's rounding statement covers the worst error of float64
polygons against exact ones with a factor of ten to spare.  MOD is left out: its plan needs a loaded module; its forms are K4's first two.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

import extrema_oracle as xo
import forms_oracle as fo


@pytest.fixture(scope="module", params=fo.EXACT_CASES)
def case(request):
    return fo.inputs(request.param)


def test_product_of_a_polygon_with_itself_is_the_square():
    P = np.random.default_rng(1).standard_normal((3, 4, 6))
    assert np.array_equal(fo.product(P, P), xo.square(P))
    Q = np.random.default_rng(2).standard_normal((3, 4, 4))
    # a product with the constant 1 (degree 0) is the polygon; with (1, 1) (degree 1) its elevation, up to the weights' rounding
    assert np.array_equal(fo.product(P, np.ones((3, 4, 1))), P)
    assert np.allclose(fo.product(Q, np.ones((3, 4, 2))), fo.eo.elevate(Q), rtol=1e-15, atol=0)


def test_oracle_encloses_the_exact_extrema(case):
    c = case
    lv = c.levels()
    for b in range(c.nexact):
        ex = fo.exact_extrema(c.spec, c.x[b], c.forms, 0.25 * c.sl[b], None if c.fprm is None else c.fprm[b], None if c.knots is None else c.knots[b])
        for f in range(len(c.forms)):
            r, sl = lv[b][f], c.sl[b, f]
            lo, hi, vlo, vhi = (float(v) for v in ex[f])
            e = r["ext"]
            print(f"{c.name} problem {b} form {f}: status {r['status']}, depth {r['depth']}, most open {r['max_open']}, min in [{e[0]:.9g}, {e[1]:.9g}] exact {lo:.9g}, "
                  f"max in [{e[2]:.9g}, {e[3]:.9g}] exact {vhi:.9g}, slack {sl:.3g}")
            assert e[0] - sl <= hi and lo <= e[1] + sl, (c.name, b, f)
            assert e[2] - sl <= vhi and vlo <= e[3] + sl, (c.name, b, f)
            assert r["status"] == c.expect
            if r["status"] == fo.OK:
                assert e[1] - e[0] <= c.tol and e[3] - e[2] <= c.tol


def test_decisions_keep_their_distance(case):
    """Every comparison "plo < U - tol" / "phi > V + tol" of the float64 oracle lies at least 16 slacks of its form away from its limit, so the
    kernel, whose figures differ from the oracle's by less than a slack, decides every piece alike: the GPU tests may ask for equal status
    and npieces.  Depth and work list stay away from their limits as well (L80 is built to overflow the list at level 0).  If a seed does
    not satisfy this, the seed changes (forms_oracle.SEEDS), not the assertion."""
    c = case
    lv = c.levels()
    for b in range(c.x.shape[0]):
        for f in range(len(c.forms)):
            margin, r = fo.decision_margin(c.polys[f][b], c.kn(b, f), c.tol)
            assert r == lv[b][f]   # (the instrumented tolerance changes nothing)
            assert margin >= 16.0 * c.sl[b, f], (c.name, b, f, margin / c.sl[b, f])
            assert r["status"] == c.expect, (c.name, b, f)
            if c.expect == fo.OK:
                assert r["depth"] <= 24 and r["max_open"] <= 32, (c.name, b, f)


def test_header_rounding_statement_covers_float64_polygons(case):
    """the worst error of the float64 level-0 polygons against the exact ones, in slacks: at most 0.1"""
    c = case
    worst = 0.0
    for b in range(c.nexact):
        ex = fo.exact_polygons(c.spec, c.x[b], c.forms, None if c.fprm is None else c.fprm[b], None if c.knots is None else c.knots[b])
        for f in range(len(c.forms)):
            P = c.polys[f][b]
            err = max(abs(Fr(float(P[j, s])) - ex[f][j][s]) for j in range(P.shape[0]) for s in range(P.shape[1]))
            worst = max(worst, float(err) / c.sl[b, f])
    print(f"{c.name}: float64 polygons differ from the exact ones by at most {worst:.3g} slack")
    assert worst <= 0.1


def test_steering_case_moves():
    """K20 is the steering certificate's case (tests/test_gpu_forms.py): the certified minimum of speed^2 is positive for at least half of
    its problems (here: for all), so the bound is finite there"""
    c = fo.inputs("K20")
    ext = np.array([[r["ext"] for r in row] for row in c.levels()])
    assert 2 * (ext[:, 0, 0] > 0.0).sum() >= c.x.shape[0]
    bound = fo.fm.steering_bound(ext, 3.0)
    print("K20: certified |tan delta| bounds", np.round(bound, 2))
    assert np.isfinite(bound[ext[:, 0, 0] > 0.0]).all()
