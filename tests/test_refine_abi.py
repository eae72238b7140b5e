"""ntg_batch_refine without a GPU: the entry point is exported and declared with the argument list the callers were promised, and the
Python binding offers it as Plan.refine."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_refine$", syms, re.M), "ntg_batch_refine is not exported"
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_refine\(([^;]*)\);", hdr)
    assert m, "ntg_batch_refine is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == "const ntg_plan *from, const ntg_plan *to, int batch, const double *d_x_from, double *d_x_to, void *stream"


def test_plan_refine_exists(built):
    from ntg_amd import api
    assert callable(getattr(api.Plan, "refine", None))
    assert api.lib().ntg_batch_refine.argtypes is not None and len(api.lib().ntg_batch_refine.argtypes) == 6
