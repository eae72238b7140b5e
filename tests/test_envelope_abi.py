"""ntg_batch_envelope without a GPU: the entry point is exported and declared with its argument list, the definition's key sentences are in
the header, the ctypes binding carries its argument types, Plan.envelope and envelope_pieces exist, and the argument errors that need no
device answer as documented."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_envelope$", syms, re.M), "ntg_batch_envelope is not exported"
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_envelope\(([^;]*)\);", hdr)
    assert m, "ntg_batch_envelope is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == ("const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper, "
                    "double *d_lo, double *d_hi, double *d_row_lo, double *d_row_hi, double *d_viol, int *d_where, void *stream")
    assert re.search(r"#define NTG_ENVELOPE_MAX_NSUB 6\b", hdr)
    assert re.search(r"^ \*   ntg_batch_envelope\s+nothing in the reference", hdr, re.M)   # the line that says which reference interface it stands next to


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("piece q = (j << nsub) + i",
                     "npc = (max_o l_o) << nsub",
                     "the blossom of the spline at (a_j repeated k-1-i, b_j repeated i)",
                     "beta'_i = d / (b_j - a_j) * (beta_{i+1} - beta_i)",
                     "by de Casteljau at the dyadic ends of the piece",
                     "lo = +inf and hi = -inf, an empty set",
                     "b'_i = i/(d+1) b_{i-1} + (1 - i/(d+1)) b_i",
                     "the row's own Bezier polygon, not interval arithmetic",
                     "max(l - row_lo, row_hi - u, 0)",
                     "smallest row * npc + piece",
                     "S = max_i |c_{o,i}| * (2 (k-1) / h_min)^r",
                     "No floating-point atomics"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    at = api.lib().ntg_batch_envelope.argtypes
    assert at is not None and list(at) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    assert callable(getattr(api.Plan, "envelope", None))
    assert api.ENVELOPE_MAX_NSUB == 6


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs"""
    from ntg_amd import api
    L = api.lib()
    assert L.ntg_batch_envelope(None, 4, None, 0, None, None, None, None, None, None, None, None, None) == -2
    assert "null plan" in L.ntg_last_error().decode()
    assert L.ntg_batch_envelope(None, 0, None, 9, None, None, None, None, None, None, None, None, None) == -2   # before the empty batch's 0


def test_envelope_pieces():
    from ntg_amd import api, configs as cf
    spec = cf.config_T()   # outputs 0, 1 on 4 intervals, output 2 on 5
    e = api.envelope_pieces(spec, 0, 1)
    assert e.shape == ((5 << 1) + 1,) and np.array_equal(e[:9], np.linspace(0.0, 2.0, 9)) and np.isnan(e[9:]).all()
    e2 = api.envelope_pieces(spec, 2, 1)
    assert np.isfinite(e2).all() and e2[0] == 0.0 and e2[-1] == spec.knots[2][-1] and np.array_equal(e2[::2], spec.knots[2])
    own = api.envelope_pieces(np.array([0.0, 1.0, 3.0]), nsub=2)   # one break sequence, e.g. a problem's own knots
    assert np.array_equal(own, [0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0])
