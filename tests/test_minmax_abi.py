"""ntg_batch_minmax without a GPU: the entry point is exported and declared with its argument list, the constants, the two structs and the
definition's key sentences are in the header, the six kernel instances are in the library, the ctypes binding carries the argument types and
its structs have the header's sizes, Plan.minmax and the constructors of ntg_amd.minmax exist and build the expected declarations, and a null
plan is an argument error before anything else."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from ntg_amd import configs as cf, forms as fm, minmax as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    assert re.search(r"\bT ntg_batch_minmax$", syms, re.M), "ntg_batch_minmax is not exported"
    for inst in ("ILi6ELi6E", "ILi6ELi11E", "ILi10ELi19E"):   # the library runs its own kernels: <KM, KP>
        assert re.search(r"minmax_shared_kernel%s" % inst, syms) and re.search(r"minmax_pp_kernel%s" % inst, syms), inst
    m = re.search(r"int ntg_batch_minmax\(([^;]*)\);", hdr)
    assert m, "ntg_batch_minmax is not declared in include/ntg_amd.h"
    assert " ".join(m.group(1).split()) == ("const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, "
                                            "int nfp, const double *d_fprm, int ngroup, const ntg_minmax_group *groups, const ntg_minmax_member *members, "
                                            "double tol, int max_depth, int sides, const double *d_glo, const double *d_ghi, "
                                            "double *d_ext, double *d_when, int *d_which, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream")
    for define in ("NTG_MINMAX_MIN 0", "NTG_MINMAX_MAX 1", "NTG_MINMAX_MAXFORMS   16", "NTG_MINMAX_MAXTERMS   40", "NTG_MINMAX_MAXGROUPS   4", "NTG_MINMAX_MAXCLAUSES  8",
                   "NTG_MINMAX_MAXMEMBERS 16"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert "typedef struct { int form, pc; double c; } ntg_minmax_member;" in hdr
    assert "typedef struct { int outer, inner, nclause, pad; int nmem[NTG_MINMAX_MAXCLAUSES]; } ntg_minmax_group;" in hdr
    assert re.search(r"^ \*   ntg_batch_minmax\s+nothing in the reference bounds a row between samples; constraints.c:119-160", hdr, re.M)
    assert hdr.index("int ntg_batch_trig(") < hdr.index("Certified extrema of MIN / MAX EXPRESSIONS") < hdr.index("int ntg_batch_minmax(") < hdr.index("int ntg_batch_kincar_reverse(")


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("h_g(t) = OUTER_k INNER_{j in clause k} m_kj(t), m(t) = q_form(z(t)) + d",
                     "min and max are monotone",
                     "Forms are declared exactly as for ntg_batch_forms (form_nterms, terms, nfp, d_fprm: same arrays, same checks, same messages)",
                     "what fits the 4096-byte kernel argument: 3520 bytes",
                     "groups [ngroup] and members are HOST arrays, copied by the call; members is concatenated group after group, clause after clause",
                     "d = c + (pc >= 0 ? fprm_b[pc] : 0), one rounding",
                     "All forms named by one group belong to one basis class; different groups may use different classes",
                     "ties to the smallest index",
                     "ties to the smallest clause",
                     "-1 where the time is NaN",
                     "A member's polygon is its form's level-0 polygon by step 1 of ntg_batch_forms, bit for bit",
                     "a member with pc = -1 and c = 0.0 adds nothing",
                     "elevated to the group's degree D_g = max of its members' form degrees",
                     "plo = OUTER_k INNER_j plo_kj and phi = OUTER_k INNER_j phi_kj",
                     "exact and independent of the order",
                     "before anything else",
                     "The value at a piece end is OUTER_k INNER_j of the members' first or last points",
                     "which is recorded together with the value it belongs to",
                     "Rules 2 to 7 of ntg_batch_extrema, unchanged",
                     "there is no NONE",
                     "Every polygon of an open piece is halved with 0.5 * (a + b)",
                     "npieces counts pieces, not polygons",
                     "ext, when, status and npieces are equal under ==",
                     "Repeating that member, as two clauses of one or one clause of two, changes nothing",
                     "every operation above is odd-symmetric in round-to-nearest",
                     "slack_g = max over its members of 2^-39 (M_f + |d|)",
                     "it closes only linearly: U - plo is about slope * width",
                     "the depth needed is about log2(h * slope / tol)",
                     "ends in status DEPTH: that is the honest answer, and the enclosure returned is still valid",
                     "without scratch in HBM and without floating-point atomics",
                     "independent of the batch around a problem",
                     "batch <= 0 or ngroup == 0 returns 0 after the checks",
                     "per wavefront nC + nfp + 64 (MC * PW + 1) doubles",
                     "Four wavefronts where four fit, else two, else one; MC = 16 with PW = 19 does not fit even one"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    ip = C.POINTER(C.c_int)
    assert list(L.ntg_batch_minmax.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(api.FormTerm), C.c_int, C.c_void_p, C.c_int, C.POINTER(api.MinmaxGroup),
                                                 C.POINTER(api.MinmaxMember), C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 10
    assert [n for n, _ in api.MinmaxMember._fields_] == ["form", "pc", "c"] and C.sizeof(api.MinmaxMember) == 2 * 4 + 8 == 16   # the header's structs, member by member: no padding
    assert [n for n, _ in api.MinmaxGroup._fields_] == ["outer", "inner", "nclause", "pad", "nmem"] and C.sizeof(api.MinmaxGroup) == 4 * 4 + 8 * 4 == 48
    assert api.MinmaxMember.c.offset == 8 and api.MinmaxGroup.nmem.offset == 16
    assert callable(getattr(api.Plan, "minmax", None))
    assert (api.MINMAX_MIN, api.MINMAX_MAX) == (mm.MIN, mm.MAX) == (0, 1)
    assert (api.MINMAX_MAXFORMS, api.MINMAX_MAXTERMS, api.MINMAX_MAXGROUPS, api.MINMAX_MAXCLAUSES, api.MINMAX_MAXMEMBERS) == \
        (mm.MAXFORMS, mm.MAXTERMS, mm.MAXGROUPS, mm.MAXCLAUSES, mm.MAXMEMBERS) == (16, 40, 4, 8, 16)
    for name in ("halfplane", "polygon", "box", "corridor", "discs", "merge"):
        assert callable(getattr(mm, name, None)), name


def test_constructors():
    spec = cf._kincar_spec(1, 6, 3, 4, 21, 5.0, "kincar-2out-k6-l4")   # flag: x, x', x'', y, y', y''
    forms, (outer, inner, clauses) = mm.polygon(spec, 0, 1, [(0, 0), (1, 0), (1, 1), (0, 1)])
    assert (outer, inner) == (mm.MIN, mm.MAX) and clauses == [[(0, 0.0, -1), (1, 0.0, -1), (2, 0.0, -1), (3, 0.0, -1)]]
    normals = [(0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0)]      # outward, edge by edge
    through = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]        # ... through the edge's first vertex
    assert forms == [[fm.Term(0, -1, -1, -1, nx, px, 0.0), fm.Term(3, -1, -1, -1, ny, py, 0.0)] for (nx, ny), (px, py) in zip(normals, through)]
    assert mm.halfplane(spec, 0, 1, 0.6, 0.8, 2.0, 3.0, 4, 5) == [fm.Term(0, -1, 4, -1, 0.6, 2.0, 0.0), fm.Term(3, -1, 5, -1, 0.8, 3.0, 0.0)]
    face = lambda f, x, y: sum(t.w * ((x if t.u == 0 else y) - t.su) for t in f)
    assert max(face(f, 0.5, 0.5) for f in forms) == -0.5 and max(face(f, 2.0, 0.5) for f in forms) == 1.0      # inside, outside
    assert all(t.pu == (7 if t.u == 0 else 8) for f in mm.polygon(spec, 0, 1, [(0, 0), (1, 0), (0, 1)], centre_params=(7, 8))[0] for t in f)
    for bad in ([(0, 0), (0, 1), (1, 1), (1, 0)],                    # clockwise
                [(0, 0), (2, 0), (1, 0.5), (2, 2), (0, 2)],          # not convex
                [(0, 0), (1, 0)], [(0, 0), (0, 0), (1, 0), (0, 1)], [(math.cos(0.3 * i), math.sin(0.3 * i)) for i in range(17)]):
        with pytest.raises(ValueError):
            mm.polygon(spec, 0, 1, bad)
    bf, bg = mm.box(spec, 0, 1, 1.0, 2.0, 3.0, 0.5)
    assert bg == (mm.MIN, mm.MAX, [[(0, 0.0, -1), (1, 0.0, -1), (2, 0.0, -1), (3, 0.0, -1)]])
    assert [(t.w, t.su) for t in bf[1]] == [(1.0, 4.0), (0.0, 1.5)] and [(t.w, t.su) for t in bf[3]] == [(-1.0, -2.0), (-0.0, 2.5)]
    cfm, cg = mm.corridor(spec, 0, 1, [(1.0, 2.0, 3.0, 0.5), (5.0, 2.0, 2.0, 1.0, 0.2)])
    assert len(cfm) == 8 and cfm[:4] == bf and cg == (mm.MIN, mm.MAX, [[(m, 0.0, -1) for m in range(4)], [(m, 0.0, -1) for m in range(4, 8)]])
    df, dg = mm.discs(spec, 0, 1, [(1.0, 2.0, 3.0), (4.0, 5.0, 0.5, 0, 1)])
    assert dg == (mm.MIN, mm.MIN, [[(0, -9.0, -1), (1, -0.25, -1)]])
    assert df == [fm.square(0, 1.0) + fm.square(3, 2.0), fm.square(0, 4.0, 0) + fm.square(3, 5.0, 1)]
    forms, groups = mm.merge((bf, bg), (cfm, cg), (df, dg))
    assert forms == cfm + df and groups[0] == bg and groups[1] == cg         # the box is the corridor's first: its forms are kept once
    assert groups[2] == (mm.MIN, mm.MIN, [[(8, -9.0, -1), (9, -0.25, -1)]])
    with pytest.raises(ValueError):
        mm.merge(*[mm.polygon(spec, 0, 1, [(i, 0), (i + 1, 0), (i, 1)]) for i in range(6)])
    with pytest.raises(ValueError):
        mm.corridor(spec, 0, 1, [(float(i), 0.0, 1.0, 1.0) for i in range(5)])


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs, and before the empty declaration's 0"""
    from ntg_amd import api
    L = api.lib()
    for ngroup in (2, 0):
        assert L.ntg_batch_minmax(None, 4, None, 1, None, None, 0, None, ngroup, None, None, 1e-9, 30, 3, None, None, None, None, None, None, None, None, None, None) == -2
        assert "null plan" in L.ntg_last_error().decode()
