"""ntg_batch_check without a GPU: the entry point is exported and declared, and a family module built from include/ntg_amd_family.hpp
carries its own check launcher in the descriptor the library checks at load."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = os.path.join(ROOT, "ntg_amd", "modules")


class Desc(C.Structure):
    """ntg_family_module_desc of ntg_amd/csrc/family_module.hpp"""
    _fields_ = [("abi", C.c_ulonglong), ("sizes", C.c_int * 6), ("name", C.c_char_p), ("dm", C.c_int), ("nn", C.c_int * 3), ("nout", C.c_int),
                ("launch_eval", C.c_void_p), ("launch_sqp", C.c_void_p), ("nparam", C.c_int), ("nparam_bp", C.c_int),
                ("sizeof_check_args", C.c_int), ("launch_check", C.c_void_p)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return {m: family.build_module(os.path.join(MODULES, m + ".hip")) for m in ("unicycle", "tracking")}


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_check$", syms, re.M), "ntg_batch_check is not exported"
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_check\(([^;]*)\);", hdr)
    assert m, "ntg_batch_check is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == ("const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, int ntimes, "
                    "const double *d_times, long long times_stride, double *d_viol, int *d_where, double *d_rows, void *stream")


@pytest.mark.parametrize("name", ["unicycle", "tracking"])
def test_module_descriptor_carries_a_check_launcher(built, name):
    from ntg_amd import api, build
    lib = C.CDLL(built[name])
    lib.ntg_family_module_v1.restype = C.POINTER(Desc)
    d = lib.ntg_family_module_v1().contents
    assert d.abi == int(build.abi_stamp()[:-3], 16)
    assert d.name.decode() == name
    assert d.launch_eval and d.launch_sqp and d.launch_check
    assert d.sizeof_check_args > 0
    assert api.load_family(built[name]) >= 64   # the library accepts it (a null launcher is a malformed descriptor)
    # the module holds its own instance of the kernel
    from ntg_amd import family
    asm = open(family.check_assembly_path(os.path.join(MODULES, name + ".hip")), errors="replace").read()
    assert re.search(r"\.amdhsa_kernel\s+\S*check_kernel\S*", asm)
