"""ntg_batch_extrema / ntg_plan_extrema_rows without a GPU: the entry points are exported and declared with their argument lists, the
constants and the definition's key sentences are in the header, the ctypes binding carries the argument types, Plan.extrema and
Plan.extrema_rows exist, a null plan is an argument error -- and two statements about tests/extrema_oracle.py on the very inputs the GPU
tests use: level_oracle (the definition in float64) encloses exact_extrema (rational bisection) to the slack, and it ends every flagged row
with status OK at depth <= 24 with at most 32 open pieces at any level.  Those margins to the limits of 30 and 64 mean that rounding
differences on the device cannot tip a row into DEPTH or FULL, so the GPU tests may leave out no row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extrema_oracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_points_are_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    for name, want in (("ntg_plan_extrema_rows", "const ntg_plan *p, int *flags"),
                       ("ntg_batch_extrema", "const ntg_plan *p, int batch, const double *d_x, double tol, int max_depth, int sides, "
                                             "const double *d_lower, const double *d_upper, double *d_ext, double *d_when, int *d_status, int *d_npieces, "
                                             "double *d_viol, int *d_where, void *stream")):
        assert re.search(r"\bT %s$" % name, syms, re.M), name + " is not exported"
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, name + " is not declared in include/ntg_amd.h"
        assert " ".join(m.group(1).split()) == want
    for define in ("NTG_EXTREMA_MAX_DEPTH 30", "NTG_EXTREMA_CAP 64", "NTG_EXTREMA_OK 0", "NTG_EXTREMA_DEPTH 1", "NTG_EXTREMA_FULL 2", "NTG_EXTREMA_NAN 3",
                   r"NTG_EXTREMA_NONE \(-1\)"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert re.search(r"^ \*   ntg_batch_extrema\s+nothing in the reference looks for a row's extremum between samples", hdr, re.M)


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("nrow = nltc + nnltc, the linear trajectory rows first",
                     "A linear row has flag 1 when the outputs it names (non-zero ltc[i][v]) belong to one basis class",
                     "A nonlinear row has the flag ntg_plan_sos_rows gives it",
                     "{min_lo, min_hi, max_lo, max_hi}",
                     "The level-0 pieces are the l knot intervals of the row's basis class",
                     "at nsub = 0, piece j, formed by the same sequence of operations",
                     "bit for bit",
                     "kn[j] + hh[j] * ((double)i / (double)(1 << lambda))",
                     "an end at local parameter 1 takes kn[j + 1]",
                     "On equal values the smaller time wins",
                     "(sides & 1) and plo < U - tol, or (sides & 2) and phi > V + tol",
                     "No open piece: status OK, stop",
                     "lambda == max_depth: status DEPTH, the open pieces retire, stop",
                     "More than NTG_EXTREMA_CAP open pieces: status FULL, they retire, stop",
                     "each new point is 0.5 * (a + b), the two end points of a polygon are carried over, not recomputed",
                     "min_lo = Rlo, min_hi = U, max_lo = V, max_hi = Rhi",
                     "With status OK and the side asked for, min_hi - min_lo <= tol",
                     "A NaN in any plo / phi makes all four numbers and both times NaN, with status NAN",
                     "(-inf, +inf, -inf, +inf), times NaN, status NONE, npieces 0",
                     "attained = max(l - min_hi, max_lo - u, 0)",
                     "certified = max(l - min_lo, max_hi - u, 0)",
                     "2^-39 * sum_t S_t^2",
                     "without scratch in HBM and without floating-point atomics"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    assert list(L.ntg_batch_extrema.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
    assert list(L.ntg_plan_extrema_rows.argtypes) == [C.c_void_p, C.POINTER(C.c_int)]
    assert callable(getattr(api.Plan, "extrema", None)) and callable(getattr(api.Plan, "extrema_rows", None))
    assert (api.EXTREMA_MAX_DEPTH, api.EXTREMA_CAP) == (30, 64)
    assert (api.EXTREMA_OK, api.EXTREMA_DEPTH, api.EXTREMA_FULL, api.EXTREMA_NAN, api.EXTREMA_NONE) == (xo.OK, xo.DEPTH, xo.FULL, xo.NAN, xo.NONE)


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs"""
    from ntg_amd import api
    L = api.lib()
    assert L.ntg_batch_extrema(None, 4, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None) == -2
    assert "null plan" in L.ntg_last_error().decode()
    assert L.ntg_batch_extrema(None, 0, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None) == -2   # before the empty batch's 0
    assert L.ntg_plan_extrema_rows(None, None) == -2


def test_oracle_flags():
    assert xo.flags(xo.inputs("O4").spec).tolist() == [1]
    assert xo.flags(xo.inputs("OF5").spec).tolist() == [1, 1, 1]
    assert xo.flags(xo.inputs("D8").spec).tolist() == [1, 1]
    assert xo.flags(xo.inputs("K3").spec).tolist() == [1, 1, 1]
    assert xo.flags(xo.inputs("T3").spec).tolist() == [1, 1, 0]
    from ntg_amd import configs as cf
    assert xo.flags(cf.config_T()).tolist() == [0, 0, 0]   # the linear row names outputs of two basis classes, and so does nonlinear row 0


@pytest.mark.parametrize("name", xo.CASES)
def test_level_oracle_encloses_the_exact_extrema(name):
    c = xo.inputs(name)
    worst = 0.0
    for b in range(c.nexact):
        ex = xo.exact_polygons(c.spec, c.x[b], None if c.prm is None else c.prm[b], None if c.knots is None else c.knots[b])
        for r, (flag, o0, *_) in enumerate(xo.row_table(c.spec)):
            if not flag:
                continue
            s = c.sl[b, r]
            elo, ehi, Elo, Ehi = (float(v) for v in xo.exact_extrema(ex[r], s / 8))
            assert ehi - elo <= s / 8 and Ehi - Elo <= s / 8
            got = xo.level_oracle(c.polys[r][b], c.kn(b, o0), c.tol)
            mlo, mhi, Mlo, Mhi = got["ext"]
            assert got["status"] == xo.OK
            worst = max(worst, (mlo - ehi) / s, (elo - mhi) / s, (Mlo - Ehi) / s, (Elo - Mhi) / s)
            assert mhi - mlo <= c.tol and Mhi - Mlo <= c.tol
    print(f"{name}: the exact extrema outside level_oracle's enclosures by at most {worst:.3g} slack")
    assert worst <= 1.0


@pytest.mark.parametrize("name", xo.CASES)
def test_inputs_keep_their_distance_from_the_limits(name):
    c = xo.inputs(name)
    depth = nopen = 0
    for r, (flag, o0, *_) in enumerate(xo.row_table(c.spec)):
        if not flag:
            continue
        for b in range(c.x.shape[0]):
            for sides in (1, 3):
                got = xo.level_oracle(c.polys[r][b], c.kn(b, o0), c.tol, sides=sides)
                assert got["status"] == xo.OK, (name, r, b)
                depth, nopen = max(depth, got["depth"]), max(nopen, got["max_open"])
    print(f"{name}: tol {c.tol:.3g}, deepest level {depth}, most open pieces at a level {nopen}")
    assert depth <= 24 and nopen <= 32
