"""ntg_batch_forms without a GPU: the entry point is exported and declared with its argument list, the constants, the term struct and the
definition's key sentences are in the header, the ctypes binding carries the argument types, Plan.forms and the constructors of
ntg_amd.forms exist and build the expected term lists on a kincar spec, and a null plan is an argument error, also with no forms."""
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
    assert re.search(r"\bT ntg_batch_forms$", syms, re.M), "ntg_batch_forms is not exported"
    m = re.search(r"int ntg_batch_forms\(([^;]*)\);", hdr)
    assert m, "ntg_batch_forms is not declared in include/ntg_amd.h"
    assert " ".join(m.group(1).split()) == ("const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, "
                                            "int nfp, const double *d_fprm, double tol, int max_depth, int sides, const double *d_flo, const double *d_fhi, "
                                            "double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream")
    for define in ("NTG_FORM_MAXFORMS 8", "NTG_FORM_MAXTERMS 8"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert re.search(r"typedef struct \{ int u, v, pu, pv; double w, su, sv; \} ntg_form_term;", hdr)
    assert re.search(r"^ \*   ntg_batch_forms\s+nothing in the reference bounds a function of the flag between samples", hdr, re.M)
    assert hdr.index("int ntg_batch_separation(") < hdr.index("Certified extrema of QUADRATIC FORMS") < hdr.index("int ntg_batch_forms(")


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("form_nterms [nform] and terms are HOST arrays, copied by the call",
                     "terms is concatenated form after form",
                     "term_t = w (z[u] - a)(z[v] - b) when v >= 0",
                     "term_t = w (z[u] - a) when v == -1 (sv and pv are then ignored)",
                     "a = su + (pu >= 0 ? fprm_b[pu] : 0) and b = sv + (pv >= 0 ? fprm_b[pv] : 0)",
                     "ntg_plan_set_params is neither needed nor read",
                     "No family callback runs",
                     "All entries a form names must belong to one basis class",
                     "A constant offset is the caller's business",
                     "a derivative of order >= k is the single point 0 with d = 0",
                     "g_m = sum_{i + j = m} W_{d,e}[i][j] * p_i * q_j, i ascending, W_{d,e}[i][j] = C(d,i) C(e,j) / C(d+e, i+j)",
                     "the division is the one rounding",
                     "W_{d,d} is therefore bit-equal to the W_d of ntg_batch_envelope_sos",
                     "A square term has v == u, pu == pv and su == sv bitwise",
                     "the same level-0 polygon, bit for bit, as the equivalent sum-of-squares row of ntg_batch_extrema",
                     "The term's polygon is w * g_m with one rounding",
                     "terms in declared order",
                     "Every form is certified: there is no status NONE and no partial-certificate refusal",
                     "a form with both bounds absent contributes 0",
                     "certified == 0 certifies every declared form over the whole horizon",
                     "The slack of a form is 2^-39 * sum_t |w_t| S_u S_v, with S_v = 1 for a linear term",
                     "the batch must be the grids'",
                     "without scratch in HBM and without floating-point atomics",
                     "independent of the batch around a problem"):
        assert sentence in hdr, sentence
    # the two statements about the family declarations stay, each with its pointer to the new call
    for sentence in ("Squares only: no weights, no bilinear terms (ntg_batch_forms certifies what this excludes",
                     "Loaded modules declare nothing: the module descriptor has no field for it yet, so every row of a module family counts as undeclared (ntg_batch_forms"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    ip = C.POINTER(C.c_int)
    assert list(L.ntg_batch_forms.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(api.FormTerm), C.c_int, C.c_void_p, C.c_double, C.c_int,
                                                C.c_int] + [C.c_void_p] * 9
    assert [(n, t) for n, t in api.FormTerm._fields_] == [("u", C.c_int), ("v", C.c_int), ("pu", C.c_int), ("pv", C.c_int), ("w", C.c_double), ("su", C.c_double),
                                                          ("sv", C.c_double)]
    assert C.sizeof(api.FormTerm) == 40
    assert callable(getattr(api.Plan, "forms", None))
    assert (api.FORM_MAXFORMS, api.FORM_MAXTERMS) == (fm.MAXFORMS, fm.MAXTERMS) == (8, 8)
    for name in ("entry", "square", "product", "linear", "speed2", "cross", "ellipse", "steering_bound"):
        assert callable(getattr(fm, name, None)), name


def test_constructors_on_a_kincar_spec():
    spec = cf._kincar_spec(2, 6, 3, 4, 21, 5.0, "kincar-4out-k6-l4")   # flag: x1 x1' x1'' y1 y1' y1'' x2 ...
    T = fm.Term
    assert [fm.entry(spec, o, r) for o, r in ((0, 0), (0, 2), (1, 1), (3, 0))] == [0, 2, 4, 9]
    for o, r in ((4, 0), (-1, 0), (0, 3), (0, -1)):
        with pytest.raises(ValueError):
            fm.entry(spec, o, r)
    assert fm.square(4, shift=0.5, param=2, w=3.0) == [T(4, 4, 2, 2, 3.0, 0.5, 0.5)]
    assert fm.product(1, 5, w=-2.0, su=0.1, sv=0.2, pu=0, pv=1) == [T(1, 5, 0, 1, -2.0, 0.1, 0.2)]
    assert fm.linear(3, 0.8, shift=1.5, param=0) == [T(3, -1, 0, -1, 0.8, 1.5, 0.0)]
    assert fm.speed2(spec, (2, 3)) == [T(7, 7, -1, -1, 1.0, 0.0, 0.0), T(10, 10, -1, -1, 1.0, 0.0, 0.0)]
    assert fm.cross(spec, (0, 1), (1, 1)) == [T(1, 5, -1, -1, 1.0, 0.0, 0.0), T(4, 2, -1, -1, -1.0, 0.0, 0.0)]   # x' y'' - y' x''
    assert fm.cross(spec, (2, 0), (3, 0)) == [T(6, 10, -1, -1, 1.0, 0.0, 0.0), T(9, 7, -1, -1, -1.0, 0.0, 0.0)]   # x y' - y x'
    assert fm.ellipse(spec, 0, 1, 2.0, 3.0, 1, 2) == [T(0, 0, 1, 1, 0.25, 0.0, 0.0), T(3, 3, 2, 2, 1.0 / 9.0, 0.0, 0.0)]
    # |tan delta| <= L N / m^1.5 with N = max(|min_lo|, |max_hi|) of the cross form and m = min_lo of speed^2; no statement where m <= 0
    ext = np.array([[[4.0, 4.1, 9.0, 9.1], [-16.0, -15.0, 2.0, 3.0]], [[0.0, 0.1, 1.0, 1.1], [-1.0, -1.0, 1.0, 1.0]], [[1.0, 1.0, 1.0, 1.0], [-1.0, 0.0, 0.0, 5.0]]])
    assert fm.steering_bound(ext, 3.0).tolist() == [3.0 * 16.0 / 8.0, math.inf, 15.0]
    assert fm.steering_bound(ext[:, ::-1], 2.0, speed_form=1, cross_form=0).tolist() == [2.0 * 16.0 / 8.0, math.inf, 10.0]


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs, and before the empty declaration's 0"""
    from ntg_amd import api
    L = api.lib()
    for nform in (2, 0):
        assert L.ntg_batch_forms(None, 4, None, nform, None, None, 0, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None) == -2
        assert "null plan" in L.ntg_last_error().decode()
