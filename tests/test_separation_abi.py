"""ntg_batch_separation without a GPU: the entry point is exported and declared with its argument list, the constants and the definition's
key sentences are in the header, the ctypes binding carries the argument types, Plan.separation and the constants exist, and a null plan
is an argument error, also with no pairs."""
import ctypes as C
import os
import re
import subprocess

import pytest

import separation_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    assert re.search(r"\bT ntg_batch_separation$", syms, re.M), "ntg_batch_separation is not exported"
    m = re.search(r"int ntg_batch_separation\(([^;]*)\);", hdr)
    assert m, "ntg_batch_separation is not declared in include/ntg_amd.h"
    assert " ".join(m.group(1).split()) == ("const ntg_plan *p, int batch, const double *d_x, int nbody, int ndim, const int *body_outs, int deriv, "
                                            "int npairs, const int *d_pairs, const double *d_sep, double tol, int max_depth, "
                                            "double *d_min, double *d_when, int *d_status, int *d_npieces, double *d_viol, void *stream")
    for define in ("NTG_SEP_MAXDIM 4", r"NTG_SEP_BADPAIR \(-2\)"):
        assert re.search(r"#define %s(?!\w)" % define, hdr), define
    assert re.search(r"#define NTG_SOS_MAXTERMS 4(?!\w)", hdr)   # NTG_SEP_MAXDIM is that figure
    assert re.search(r"^ \*   ntg_batch_separation\s+nothing in the reference compares two trajectories", hdr, re.M)
    assert hdr.index("int ntg_batch_extrema(") < hdr.index("Certified closest approach of PAIRS") < hdr.index("int ntg_batch_separation(")


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("body_outs is a HOST array [nbody][ndim], copied by the call",
                     "d_pairs is a device array [npairs][4] of {a, b, ga, gb}",
                     "The kernel checks 0 <= a, b < batch and 0 <= ga, gb < nbody before it reads anything of the pair",
                     "it never causes a read outside d_x",
                     "s2 = sep * sep, one rounding",
                     "NULL means s2 = +inf",
                     "delta_t[i] = x[a][iC[oa_t] + i] - x[b][iC[ob_t] + i]",
                     "one IEEE subtraction per coefficient",
                     "c(t) = sum_t (D^deriv delta_t(t))^2",
                     "{dimension t, derivative deriv, shift 0, no parameter}",
                     "bit-identical to that of ntg_batch_extrema at sides = 1",
                     "a piece is open iff plo < U - tol and not plo >= s2",
                     "min_lo = Rlo, min_hi = U (an attained value)",
                     "With status OK, min_lo >= min(min_hi - tol, s2)",
                     "attained = max(s2 - min_hi, 0)",
                     "certified = max(s2 - min_lo, 0)",
                     "A NaN s2 makes both figures NaN",
                     "S_t = max_i (|x_a,i| + |x_b,i|) * (2 (k - 1) / h_min)^deriv",
                     "the result of a pair does not depend on the other pairs or on the batch",
                     "Per-problem parameters are ignored",
                     "without scratch in HBM and without floating-point atomics"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    ip = C.POINTER(C.c_int)
    assert list(L.ntg_batch_separation.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                                     C.c_int] + [C.c_void_p] * 6
    assert callable(getattr(api.Plan, "separation", None))
    assert (api.SEP_MAXDIM, api.SEP_BADPAIR) == (po.MAXDIM, po.BADPAIR) == (4, -2)


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs, and before the empty pair list's 0"""
    from ntg_amd import api
    L = api.lib()
    for npairs in (4, 0):
        assert L.ntg_batch_separation(None, 4, None, 1, 2, None, 0, npairs, None, None, 1e-9, 30, None, None, None, None, None, None) == -2
        assert "null plan" in L.ntg_last_error().decode()
