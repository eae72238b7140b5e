"""The numpy / scipy statement of ntg_batch_envelope's definition (tests/envelope_oracle.py) against scipy's BSpline itself, without a GPU:
the hull of the control points encloses the spline's samples on every piece, is exact where the entry is at most linear, shrinks when
the pieces are halved, and its excess over the sampled range falls as the definition promises.

Slack: 2^-42 max|c| (2 (k - 1) / h_min)^r, the rounding statement of include/ntg_amd.h.
Shapes (k, mult, l): those of the definition's prototype, seed fixed, coefficients of size 0.3.
"""
import numpy as np
import pytest

import envelope_oracle as eo
from ntg_amd import configs as cf

SHAPES = [(5, 3, 2), (6, 3, 20), (8, 4, 40), (4, 2, 3)]
NB = 3


def problem(k, m, l, seed=20261018):
    rng = np.random.default_rng(seed + 100 * k + l)
    brk = np.linspace(0.0, 5.0, l + 1)
    if l == 3:
        brk = np.array([0.0, 0.7, 3.1, 5.0])   # one shape on uneven breaks
    c = 0.3 * rng.standard_normal((NB, l * (k - m) + m))
    return brk, c


def slack(brk, k, c, r):
    return eo.SLACK * np.abs(c).max(axis=1) * (2.0 * (k - 1) / np.diff(brk).min()) ** r


@pytest.mark.parametrize("k,m,l", SHAPES)
@pytest.mark.parametrize("nsub", [0, 2])
def test_hull_encloses_the_samples(k, m, l, nsub):
    brk, c = problem(k, m, l)
    polys = eo.piece_polygons(brk, k, m, c, 3, nsub)
    for r in range(3):
        lo, hi = eo.hull(polys[r])
        v = eo.sample_piece(brk, k, m, c, r, nsub, 257)
        sl = slack(brk, k, c, r)[:, None]
        below, above = (lo - v.min(axis=2)) / sl, (v.max(axis=2) - hi) / sl
        print(f"k {k} l {l} nsub {nsub} r {r}: samples outside the hull by at most {max(below.max(), above.max()):.3g} slack")
        assert (below <= 1.0).all() and (above <= 1.0).all()


@pytest.mark.parametrize("k,m,l", [(4, 2, 3), (5, 3, 2)])
def test_exact_where_the_entry_is_at_most_linear(k, m, l):
    brk, c = problem(k, m, l)
    polys = eo.piece_polygons(brk, k, m, c, k, 1)
    assert len(polys) == k and polys[k - 1].shape[-1] == 1 and polys[k - 2].shape[-1] == 2
    for r in (k - 2, k - 1):
        lo, hi = eo.hull(polys[r])
        v = eo.sample_piece(brk, k, m, c, r, 1, 257)
        sl = slack(brk, k, c, r)[:, None]
        assert (np.abs(lo - v.min(axis=2)) <= sl).all() and (np.abs(hi - v.max(axis=2)) <= sl).all()


@pytest.mark.parametrize("k,m,l", SHAPES)
def test_halving_the_pieces_shrinks_the_hull(k, m, l):
    brk, c = problem(k, m, l)
    for nsub in (0, 1, 2):
        coarse, fine = eo.piece_polygons(brk, k, m, c, 3, nsub), eo.piece_polygons(brk, k, m, c, 3, nsub + 1)
        for r in range(3):
            lo0, hi0 = eo.hull(coarse[r]); lo1, hi1 = eo.hull(fine[r])
            sl = slack(brk, k, c, r)[:, None]
            lo1 = lo1.reshape(NB, -1, 2); hi1 = hi1.reshape(NB, -1, 2)   # the two halves of every coarse piece
            assert (lo1.min(axis=2) >= lo0 - sl).all() and (hi1.max(axis=2) <= hi0 + sl).all()


@pytest.mark.parametrize("k,m,l", SHAPES)
def test_excess_over_the_sampled_range_falls_with_nsub(k, m, l):
    """theory: 1/64 from nsub 0 to 3 asymptotically (quadratic in the piece length); asked for: 1/8"""
    brk, c = problem(k, m, l)
    for r in range(3):
        if k - 1 - r < 2:
            continue
        ex = []
        for nsub in (0, 3):
            lo, hi = eo.hull(eo.piece_polygons(brk, k, m, c, 3, nsub)[r])
            v = eo.sample_piece(brk, k, m, c, r, nsub, 257)
            ex.append(((hi - lo) - (v.max(axis=2) - v.min(axis=2))).max())
        print(f"k {k} l {l} r {r}: excess {ex[0]:.3g} -> {ex[1]:.3g}, ratio {ex[1] / ex[0]:.3g}")
        assert ex[0] > 0 and ex[1] <= ex[0] / 8


def test_spec_level_layout_padding_and_rows():
    """config_T: outputs of two shapes; the shorter outputs' pieces past their own are the empty set; a row is the combination of its
    entries' polygons and encloses the combination of their samples"""
    spec = cf.config_T()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, spec.nC))
    lo, hi = eo.entry_envelope(spec, x, 1)
    npc = max(spec.kninterv) << 1
    assert lo.shape == (2, spec.nz, npc)
    own = spec.kninterv[0] << 1
    assert np.isposinf(lo[:, :6, own:]).all() and np.isneginf(hi[:, :6, own:]).all() and np.isfinite(lo[:, 6:]).all() and np.isfinite(lo[:, :6, :own]).all()
    # a row on the two outputs of one class: x0' - x1' + 0.5 x1''
    import dataclasses
    ltc = np.zeros((1, spec.nz)); ltc[0, 1] = 1.0; ltc[0, 4] = -1.0; ltc[0, 5] = 0.5
    s2 = dataclasses.replace(spec, ltc=ltc)
    rlo, rhi = eo.row_envelope(s2, x, 1)
    sl = eo.row_slack(s2, x)[:, :1]
    sls = eo.coef_slices(spec)
    smp = [eo.sample_piece(spec.knots[o], spec.order[o], spec.mult[o], x[:, sls[o]], r, 1, 33) for o, r in ((0, 1), (1, 1), (1, 2))]
    v = smp[0] - smp[1] + 0.5 * smp[2]
    assert (rlo[:, 0, :own] <= v.min(axis=2) + sl).all() and (rhi[:, 0, :own] >= v.max(axis=2) - sl).all()
    assert np.isposinf(rlo[:, 0, own:]).all()
    # the row's own polygon is tighter than the sum of its entries' hulls
    wide = (hi[:, 1] - lo[:, 1]) + (hi[:, 4] - lo[:, 4]) + 0.5 * (hi[:, 5] - lo[:, 5])
    assert ((rhi - rlo)[:, 0, :own] <= wide[:, :own] + sl).all() and ((rhi - rlo)[:, 0, :own] < 0.9 * wide[:, :own]).any()
    lower = np.full((2, spec.nbounds), -1e20); upper = np.full((2, spec.nbounds), 1e20)
    upper[0, spec.nlic] = rhi[0, 0, :own].max() - 0.1
    viol, where = eo.violation(s2, rlo, rhi, lower, upper)
    assert viol[1] == 0 and tuple(where[1]) == (-1, -1) and abs(viol[0] - 0.1) < 1e-12 and tuple(where[0]) == (0, int(np.argmax(rhi[0, 0, :own])))
