"""ntg_batch_ratios without a GPU: the entry point is exported and declared with its argument list, the constants, the ratio struct and the
definition's key sentences are in the header, the ctypes binding carries the argument types, Plan.ratios and the constructors of
ntg_amd.forms exist and build the expected ratios, and the refusals that come before any device is touched are argument errors."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ntg_amd import configs as cf, forms as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    assert re.search(r"\bT ntg_batch_ratios$", syms, re.M), "ntg_batch_ratios is not exported"
    for inst in ("ILi6ELi13E", "ILi6ELi25E", "ILi10ELi25E"):   # the library runs its own kernels: <KM, KR>
        assert re.search(r"ratios_shared_kernel%s" % inst, syms) and re.search(r"ratios_pp_kernel%s" % inst, syms), inst
    m = re.search(r"int ntg_batch_ratios\(([^;]*)\);", hdr)
    assert m, "ntg_batch_ratios is not declared in include/ntg_amd.h"
    assert " ".join(m.group(1).split()) == ("const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, "
                                            "int nfp, const double *d_fprm, int nratio, const ntg_ratio *ratios, double tol, int max_depth, int sides, "
                                            "const double *d_rlo, const double *d_rhi, double *d_ext, double *d_when, int *d_status, int *d_npieces, "
                                            "double *d_viol, int *d_where, void *stream")
    for define in ("NTG_RATIO_MAXRATIOS  4", "NTG_RATIO_MAXFACTORS 4", "NTG_RATIO_MAXDEG     24", "NTG_RATIO_POLE       4"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert re.search(r"typedef struct \{ int nnum, nden; int num\[NTG_RATIO_MAXFACTORS\], den\[NTG_RATIO_MAXFACTORS\]; \} ntg_ratio;", hdr)
    assert re.search(r"^ \*   ntg_batch_ratios\s+nothing in the reference bounds the steering angle between samples", hdr, re.M)
    assert hdr.index("int ntg_batch_forms(") < hdr.index("Certified extrema of RATIOS") < hdr.index("int ntg_batch_ratios(")


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("N / Q = sum_i (n_i / d_i) (d_i B_i / sum_j d_j B_j) is a convex combination of the quotients n_i / d_i",
                     "the end quotients are attained values",
                     "Forms are declared exactly as for ntg_batch_forms",
                     "ratios [nratio] is a HOST array, copied by the call",
                     "nnum == 0 is the numerator 1, nden == 0 the denominator 1",
                     "Every form a ratio names must belong to one basis class; different ratios may use different classes",
                     "The polygon F_f of every form named is step 1 of ntg_batch_forms, bit for bit",
                     "G = F_{num[0]}; G = G (x) F_{num[a]}, a ascending",
                     "g_m = sum_{i + j = m} W_{d,e}[i][j] * G_i * F_j, i ascending",
                     "the numerator an exact integer (below 2^53: at most C(24,12)^2), the division its one rounding",
                     "An empty side is the single point 1.0",
                     "the lower side is elevated to DR = max(dN, dD)",
                     "rho_i = n_i / d_i by one IEEE division",
                     "Otherwise plo = -inf and phi = +inf: the piece is open on every side asked for",
                     "An end with d <= 0 is never taken and marks the ratio POLE",
                     "NAN takes precedence over POLE",
                     "Both polygons of an open piece are halved with 0.5 * (a + b)",
                     "npieces counts pairs",
                     "a POLE ratio with a bound present gives certified = +inf and attained = 0",
                     "eps_side = prod_f m_f * (sum_f delta_f / m_f + 2^-43)",
                     "a quotient rho carries at most (eps_N + |rho| eps_D) / (d_min - eps_D)",
                     "A certificate is claimed only where d_min > eps_D",
                     "without scratch in HBM and without floating-point atomics",
                     "independent of the batch around a problem",
                     "batch <= 0 or nratio == 0 returns 0 after the checks"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    ip = C.POINTER(C.c_int)
    assert list(L.ntg_batch_ratios.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(api.FormTerm), C.c_int, C.c_void_p, C.c_int, C.POINTER(api.Ratio),
                                                 C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
    assert [n for n, _ in api.Ratio._fields_] == ["nnum", "nden", "num", "den"] and C.sizeof(api.Ratio) == 40
    assert callable(getattr(api.Plan, "ratios", None))
    assert (api.RATIO_MAXRATIOS, api.RATIO_MAXFACTORS, api.RATIO_MAXDEG, api.RATIO_POLE) == (fm.MAXRATIOS, fm.MAXFACTORS, 24, 4) == (4, 4, 24, 4)
    for name in ("ratio", "curvature2", "lateral_accel2", "steering_tan_max"):
        assert callable(getattr(fm, name, None)), name


def test_constructors():
    spec = cf._kincar_spec(1, 6, 3, 4, 21, 5.0, "kincar-2out-k6-l4")
    assert fm.ratio([1, 1], [0, 0, 0]) == ([1, 1], [0, 0, 0]) and fm.ratio([2]) == ([2], []) and fm.ratio([], (3,)) == ([], [3])
    with pytest.raises(ValueError):
        fm.ratio([], [])
    with pytest.raises(ValueError):
        fm.ratio([0] * 5, [1])
    forms, k2 = fm.curvature2(spec, (0, 1))
    assert forms == [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1))] and k2 == ([1, 1], [0, 0, 0])   # T T / (S S S)
    forms, a2 = fm.lateral_accel2(spec, (0, 1))
    assert forms == [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1))] and a2 == ([1, 1], [0])
    # L sqrt(max_hi) where the status is OK, inf elsewhere
    out = {"ext": np.array([[[0.0, 0.0, 3.9, 4.0]], [[0.0, 0.0, 0.2, 0.25]], [[-np.inf, np.inf, -np.inf, np.inf]], [[0.0, 0.0, 1.0, 1.0]]]),
           "status": np.array([[0], [0], [4], [1]])}
    assert fm.steering_tan_max(out, 3.0).tolist() == [6.0, 1.5, math.inf, math.inf]


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs, and before the empty declaration's 0"""
    from ntg_amd import api
    L = api.lib()
    for nratio in (1, 0):
        assert L.ntg_batch_ratios(None, 4, None, 2, None, None, 0, None, nratio, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None) == -2
        assert "null plan" in L.ntg_last_error().decode()
