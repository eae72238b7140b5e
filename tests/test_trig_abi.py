"""ntg_batch_trig without a GPU: the entry point is exported and declared with its argument list, the constants, the term struct and the
definition's key sentences are in the header, the four kernel instances are in the library, the ctypes binding carries the argument types,
Plan.trig and the constructors of ntg_amd.trig exist and build the expected forms, and a null plan is an argument error before anything else."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from ntg_amd import configs as cf, trig as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    assert re.search(r"\bT ntg_batch_trig$", syms, re.M), "ntg_batch_trig is not exported"
    for inst in ("ILi6E", "ILi10E"):   # the library runs its own kernels: <KM>
        assert re.search(r"trig_shared_kernel%s" % inst, syms) and re.search(r"trig_pp_kernel%s" % inst, syms), inst
    m = re.search(r"int ntg_batch_trig\(([^;]*)\);", hdr)
    assert m, "ntg_batch_trig is not declared in include/ntg_amd.h"
    assert " ".join(m.group(1).split()) == ("const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_trig_term *terms, "
                                            "int nfp, const double *d_fprm, double tol, int max_depth, int sides, "
                                            "const double *d_flo, const double *d_fhi, double *d_ext, double *d_when, int *d_status, int *d_npieces, "
                                            "double *d_viol, int *d_where, void *stream")
    for define in ("NTG_TRIG_MAXFORMS 8", "NTG_TRIG_MAXTERMS 4", "NTG_TRIG_MAXENT   4", "NTG_TRIG_SIN 0", "NTG_TRIG_COS 1", "NTG_TRIG_LIN 2"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert re.search(r"typedef struct \{ int kind, nent, pp, pad; int ent\[NTG_TRIG_MAXENT\]; double coef\[NTG_TRIG_MAXENT\]; double phase, w; \} ntg_trig_term;", hdr)
    assert re.search(r"^ \*   ntg_batch_trig\s+nothing in the reference bounds a row between samples; constraints.c:119-160", hdr, re.M)
    assert hdr.index("int ntg_batch_ratios(") < hdr.index("Certified extrema of SINES AND COSINES") < hdr.index("int ntg_batch_trig(")


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("h_j(z) = sum_t w_t g_t(theta_t(z)), theta_t = sum_i coef[i] * z[ent[i]] + phase + (pp >= 0 ? fprm_b[pp] : 0)",
                     "|R| <= rho^2 / 2",
                     "form_nterms [nform] and terms are HOST arrays, copied by the call",
                     "Every entry of a form belongs to one basis class",
                     "Every product and every sum below is rounded separately (no fused multiply-add)",
                     "Each entry polygon is multiplied by its coef (one rounding)",
                     "then phase + fprm_b[pp] is added to every point",
                     "D_j, the largest entry degree of the whole form (D_j <= 9)",
                     "added to the form's linear polygon Lambda, LIN terms in declared order",
                     "c_t = 0.5 * (lo_t + hi_t), rho_t = max(hi_t - c_t, c_t - lo_t), (S, C) = sincos(c_t)",
                     "T_t,m = w_t * (S + C * (Theta_t,m - c_t)) for SIN",
                     "T_t,m = w_t * (C - S * (Theta_t,m - c_t)) for COS",
                     "r = sum_t |w_t| * rho_t * rho_t * 0.5",
                     "plo = max(plo, -W) and phi = min(phi, W) with W = sum_t |w_t|",
                     "which de Casteljau carries over bit for bit",
                     "Rules 2 to 7 of ntg_batch_extrema, unchanged",
                     "Every polygon of an open piece is halved with 0.5 * (a + b)",
                     "there is no status NONE",
                     "ext, when, status and npieces are equal under ==",
                     "the device sincos is taken at 4 ulp",
                     "slack_j = 2^-39 * sum_t |w_t| (1 + A_t)",
                     "without scratch in HBM and without floating-point atomics",
                     "independent of the batch around a problem",
                     "batch <= 0 or nform == 0 returns 0 after the checks",
                     "four wavefronts, two where four do not fit"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    ip = C.POINTER(C.c_int)
    assert list(L.ntg_batch_trig.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(api.TrigTerm), C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
    assert [n for n, _ in api.TrigTerm._fields_] == ["kind", "nent", "pp", "pad", "ent", "coef", "phase", "w"]
    assert C.sizeof(api.TrigTerm) == 4 * 4 + 4 * 4 + 4 * 8 + 2 * 8 == 80   # the header's struct, member by member: no padding
    assert callable(getattr(api.Plan, "trig", None))
    assert (api.TRIG_MAXFORMS, api.TRIG_MAXTERMS, api.TRIG_MAXENT) == (tg.MAXFORMS, tg.MAXTERMS, tg.MAXENT) == (8, 4, 4)
    assert (api.TRIG_SIN, api.TRIG_COS, api.TRIG_LIN) == (tg.SIN, tg.COS, tg.LIN) == (0, 1, 2)
    for name in ("term", "sin_sum", "tip_height", "tip_x", "wall", "heading"):
        assert callable(getattr(tg, name, None)), name


def test_constructors():
    spec = cf.config_E(ninterv=4, narms=2)
    h = tg.tip_height(spec, 1)   # arm 1: outputs 3, 4, 5, flag entries 9, 12, 15
    assert h == [tg.Term(tg.SIN, (9,), (1.0,), 0.0, -1, 1.0), tg.Term(tg.SIN, (9, 12), (1.0, 1.0), 0.0, -1, 1.0), tg.Term(tg.SIN, (9, 12, 15), (1.0, 1.0, 1.0), 0.0, -1, 1.0)]
    assert tg.tip_x(spec, 1) == [t._replace(kind=tg.COS) for t in h]
    assert tg.sin_sum(spec, [3, 4, 5]) == h
    w = tg.wall(spec, 0, 3.0, 4.0, param=2)   # 3 x + 4 y = 5 sin(theta + atan2(3, 4)) summed over the links
    assert [t.ent for t in w] == [(0,), (0, 3), (0, 3, 6)] and all(t.kind == tg.SIN and t.w == 5.0 and t.pp == 2 and t.phase == math.atan2(3.0, 4.0) for t in w)
    th = 0.7
    assert abs(5.0 * math.sin(th + w[0].phase) - (3.0 * math.cos(th) + 4.0 * math.sin(th))) < 1e-14
    assert tg.heading(spec, 2) == [tg.Term(tg.LIN, (6,), (1.0,), 0.0, -1, 1.0)] and tg.heading(spec, 2, kind=tg.COS, w=2.0, deriv=1) == [tg.Term(tg.COS, (7,), (1.0,), 0.0, -1, 2.0)]
    for bad in (lambda: tg.tip_height(spec, 2), lambda: tg.term(3, [0]), lambda: tg.term(tg.SIN, [0] * 5), lambda: tg.term(tg.SIN, [0, 1], [1.0]), lambda: tg.sin_sum(spec, [])):
        with pytest.raises(ValueError):
            bad()


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs, and before the empty declaration's 0"""
    from ntg_amd import api
    L = api.lib()
    for nform in (2, 0):
        assert L.ntg_batch_trig(None, 4, None, nform, None, None, 0, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None) == -2
        assert "null plan" in L.ntg_last_error().decode()
