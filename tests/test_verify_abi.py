"""ntg_batch_verify without a GPU: the entry point is exported and declared with its argument list, the ctypes binding carries its argument
types, the argument errors that need no device answer as documented, and every family descriptor -- built in, and of the family modules
built from include/ntg_amd_family.hpp, the planted-error family of tests/modules among them -- carries its own verify launcher."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = {"unicycle": os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip"), "tracking": os.path.join(ROOT, "ntg_amd", "modules", "tracking.hip"),
           "miswired": os.path.join(ROOT, "tests", "modules", "miswired.hip")}


class Desc(C.Structure):
    """ntg_family_module_desc of ntg_amd/csrc/family_module.hpp"""
    _fields_ = [("abi", C.c_ulonglong), ("sizes", C.c_int * 6), ("name", C.c_char_p), ("dm", C.c_int), ("nn", C.c_int * 3), ("nout", C.c_int),
                ("launch_eval", C.c_void_p), ("launch_sqp", C.c_void_p), ("nparam", C.c_int), ("nparam_bp", C.c_int),
                ("sizeof_check_args", C.c_int), ("launch_check", C.c_void_p), ("sizeof_cost_args", C.c_int), ("launch_cost", C.c_void_p),
                ("sizeof_verify_args", C.c_int), ("launch_verify", C.c_void_p)]


class Family(C.Structure):
    """NtgFamily of ntg_amd/csrc/family_module.hpp (the descriptor of a built-in family, exported as ntg_fam_<name>)"""
    _fields_ = [("name", C.c_char_p), ("dm", C.c_int), ("nn", C.c_int * 3), ("nout", C.c_int), ("couple", C.c_int), ("cg", C.c_int),
                ("group_mask", C.c_ulonglong), ("free_outputs_ok", C.c_bool), ("nparam", C.c_int), ("nparam_bp", C.c_int),
                ("nparam_row", C.c_int), ("kincar_flag", C.c_bool), ("shape", C.c_void_p), ("launch_eval", C.c_void_p),
                ("launch_sqp", C.c_void_p), ("launch_check", C.c_void_p), ("launch_cost", C.c_void_p), ("launch_verify", C.c_void_p)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return {m: family.build_module(src) for m, src in SOURCES.items()}


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_verify$", syms, re.M), "ntg_batch_verify is not exported"
    assert re.search(r"\bT ntg_debug_batch_verify$", syms, re.M), "ntg_debug_batch_verify is not exported"
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_verify\(([^;]*)\);", hdr)
    assert m, "ntg_batch_verify is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == "const ntg_plan *p, int batch, const double *d_x, double *d_err, int *d_where, double *d_leak, int *d_leak_where, void *stream"
    assert re.search(r"#define NTG_VERIFY_NSLOT 6\b", hdr)
    assert "h = 2^-17 * max(1, |z_v|)" in hdr and "scale = max(1, |f(z)|, |an|, |fd|)" in hdr   # the definition is part of the contract
    assert "NO threshold inside the library" in hdr


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    at = api.lib().ntg_batch_verify.argtypes
    assert at is not None and list(at) == [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert callable(getattr(api.Plan, "verify", None))


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs"""
    from ntg_amd import api
    L = api.lib()
    assert L.ntg_batch_verify(None, 4, None, None, None, None, None, None) == -2
    assert "null plan" in L.ntg_last_error().decode()


@pytest.mark.parametrize("name", ["kincar", "vanderpol", "testfam", "obstacle", "quadrotor", "manip", "obstacle_field"])
def test_builtin_descriptor_carries_a_verify_launcher(built, name):
    from ntg_amd import api
    d = Family.in_dll(api.lib(), "ntg_fam_" + name)
    assert d.name.decode() == name
    assert d.launch_eval and d.launch_sqp and d.launch_check and d.launch_cost and d.launch_verify
    assert d.launch_verify != d.launch_cost and d.launch_verify != d.launch_check


@pytest.mark.parametrize("name", ["unicycle", "tracking", "miswired"])
def test_module_descriptor_carries_a_verify_launcher(built, name):
    from ntg_amd import api, build, family
    lib = C.CDLL(built[name])
    lib.ntg_family_module_v1.restype = C.POINTER(Desc)
    d = lib.ntg_family_module_v1().contents
    assert d.abi == int(build.abi_stamp()[:-3], 16)
    assert d.name.decode() == name
    assert d.launch_check and d.launch_cost and d.launch_verify and d.launch_verify != d.launch_cost
    assert d.sizeof_verify_args > d.sizeof_check_args   # (VerifyArgs holds the tile fields of CheckArgs)
    assert api.load_family(built[name]) >= 64   # the library accepts it (a null launcher is a malformed descriptor)
    # the module's second part holds its own instance of the kernel, next to its check and cost instances
    asm = open(family.check_assembly_path(SOURCES[name]), errors="replace").read()
    for k in ("verify_kernel", "check_kernel", "cost_kernel"):
        assert re.search(r"\.amdhsa_kernel\s+\S*" + k + r"\S*", asm), k
