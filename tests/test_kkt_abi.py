"""ntg_batch_kkt without a GPU: the entry points are exported, the header declares the call with its argument list and the size of a
result row, and the ctypes binding carries its argument types."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_points_are_exported(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_kkt$", syms, re.M), "ntg_batch_kkt is not exported"
    assert re.search(r"\bT ntg_debug_batch_kkt$", syms, re.M), "ntg_debug_batch_kkt is not exported"


def test_header_declares_the_call():
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_kkt\(([^;]*)\);", hdr)
    assert m, "ntg_batch_kkt is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == ("const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, "
                    "const double *d_clambda, double *d_res, double *d_r, void *stream")
    assert re.search(r"^#define NTG_KKT_NRES 6\s*$", hdr, re.M)


def test_binding_carries_argtypes(built):
    import ctypes as C
    from ntg_amd import api
    at = api.lib().ntg_batch_kkt.argtypes
    assert at is not None and list(at) == [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    assert callable(getattr(api.Plan, "kkt", None))
