"""ntg_batch_cost without a GPU: the entry point is exported and declared with its argument list, the ctypes binding carries its argument
types, the argument errors that need no device answer as documented, every family descriptor -- built in, and of a family module built
from include/ntg_amd_family.hpp -- carries its own cost launcher, and the quadrature helpers of ntg_amd.quadrature are exact where
they must be."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = os.path.join(ROOT, "ntg_amd", "modules")


class Desc(C.Structure):
    """ntg_family_module_desc of ntg_amd/csrc/family_module.hpp"""
    _fields_ = [("abi", C.c_ulonglong), ("sizes", C.c_int * 6), ("name", C.c_char_p), ("dm", C.c_int), ("nn", C.c_int * 3), ("nout", C.c_int),
                ("launch_eval", C.c_void_p), ("launch_sqp", C.c_void_p), ("nparam", C.c_int), ("nparam_bp", C.c_int),
                ("sizeof_check_args", C.c_int), ("launch_check", C.c_void_p), ("sizeof_cost_args", C.c_int), ("launch_cost", C.c_void_p)]


class Family(C.Structure):
    """NtgFamily of ntg_amd/csrc/family_module.hpp (the descriptor of a built-in family, exported as ntg_fam_<name>)"""
    _fields_ = [("name", C.c_char_p), ("dm", C.c_int), ("nn", C.c_int * 3), ("nout", C.c_int), ("couple", C.c_int), ("cg", C.c_int),
                ("group_mask", C.c_ulonglong), ("free_outputs_ok", C.c_bool), ("nparam", C.c_int), ("nparam_bp", C.c_int),
                ("nparam_row", C.c_int), ("kincar_flag", C.c_bool), ("shape", C.c_void_p), ("launch_eval", C.c_void_p),
                ("launch_sqp", C.c_void_p), ("launch_check", C.c_void_p), ("launch_cost", C.c_void_p)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return {m: family.build_module(os.path.join(MODULES, m + ".hip")) for m in ("unicycle", "tracking")}


def test_entry_point_is_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT ntg_batch_cost$", syms, re.M), "ntg_batch_cost is not exported"
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    m = re.search(r"int ntg_batch_cost\(([^;]*)\);", hdr)
    assert m, "ntg_batch_cost is not declared in include/ntg_amd.h"
    args = " ".join(m.group(1).split())
    assert args == ("const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, const double *d_weights, "
                    "long long times_stride, double *d_cost, double *d_vals, void *stream")
    assert re.search(r"initial and final cost functions are NOT part of the result", hdr)


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    at = api.lib().ntg_batch_cost.argtypes
    assert at is not None and list(at) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_void_p] * 3
    assert callable(getattr(api.Plan, "cost", None))


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs; without a device no plan can exist (NTG_E_NODEVICE at ntg_plan_create)"""
    from ntg_amd import api, configs as cf
    L = api.lib()
    assert L.ntg_batch_cost(None, 4, None, 8, None, None, 0, None, None, None) == -2
    assert "null plan" in L.ntg_last_error().decode()
    L.ntg_device_count.restype = C.c_int
    if L.ntg_device_count() <= 0:
        with pytest.raises(api.NtgError, match="-1"):
            api.Plan(cf.config_B(), 0)


@pytest.mark.parametrize("name", ["kincar", "vanderpol", "testfam", "obstacle", "quadrotor", "manip", "obstacle_field"])
def test_builtin_descriptor_carries_a_cost_launcher(built, name):
    from ntg_amd import api
    d = Family.in_dll(api.lib(), "ntg_fam_" + name)
    assert d.name.decode() == name
    assert d.launch_eval and d.launch_sqp and d.launch_check and d.launch_cost
    assert d.launch_cost != d.launch_check


@pytest.mark.parametrize("name", ["unicycle", "tracking"])
def test_module_descriptor_carries_a_cost_launcher(built, name):
    from ntg_amd import api, build, family
    lib = C.CDLL(built[name])
    lib.ntg_family_module_v1.restype = C.POINTER(Desc)
    d = lib.ntg_family_module_v1().contents
    assert d.abi == int(build.abi_stamp()[:-3], 16)
    assert d.name.decode() == name
    assert d.launch_check and d.launch_cost and d.sizeof_cost_args > d.sizeof_check_args   # (CostArgs holds the tile fields of CheckArgs)
    assert api.load_family(built[name]) >= 64   # the library accepts it (a null launcher is a malformed descriptor)
    # the module holds its own instance of the kernel, next to its check instance
    asm = open(family.check_assembly_path(os.path.join(MODULES, name + ".hip")), errors="replace").read()
    assert re.search(r"\.amdhsa_kernel\s+\S*cost_kernel\S*", asm) and re.search(r"\.amdhsa_kernel\s+\S*check_kernel\S*", asm)


# ---- ntg_amd.quadrature ----
BREAKS = [np.linspace(0.0, 5.0, 21), np.array([0.0, 0.3, 0.35, 2.0, 4.4, 5.0]), np.array([-1.0, 2.5])]


@pytest.mark.parametrize("bi", range(len(BREAKS)))
def test_trapezoid_is_the_plans_rule(bi):
    from ntg_amd import quadrature as q
    br = BREAKS[bi]
    t, w = q.trapezoid(br)
    assert t.dtype == np.float64 and w.dtype == np.float64 and np.array_equal(t, br)
    assert abs(w.sum() - (br[-1] - br[0])) <= 1e-14 * (br[-1] - br[0])
    f = 3.0 * br - 1.0   # exact on piecewise linear functions
    exact = 1.5 * (br[-1] ** 2 - br[0] ** 2) - (br[-1] - br[0])
    assert abs((w * f).sum() - exact) <= 1e-14 * max(1.0, abs(exact))
    t2, w2 = q.trapezoid(np.stack([br, 2.0 * br + 1.0]))   # per-problem grids
    assert t2.shape == w2.shape == (2, br.size) and np.array_equal(w2[0], w) and np.allclose(w2[1], 2.0 * w, rtol=1e-15, atol=0)


@pytest.mark.parametrize("npts", [1, 2, 3, 4, 6, 9])
@pytest.mark.parametrize("bi", range(len(BREAKS)))
def test_gauss_legendre_is_exact_to_its_degree(bi, npts):
    from ntg_amd import quadrature as q
    br = BREAKS[bi]
    t, w = q.gauss_legendre(br, npts)
    assert t.shape == w.shape == ((br.size - 1) * npts,) and t.dtype == np.float64 and w.dtype == np.float64
    assert (t > br[0]).all() and (t < br[-1]).all() and (np.diff(t) > 0).all() and (w > 0).all()
    d = 2 * npts - 1
    exact = (br[-1] ** (d + 1) - br[0] ** (d + 1)) / (d + 1)
    got = (w * t ** d).sum()
    assert abs(got - exact) <= 1e-14 * abs(exact), (got, exact)
    t2, w2 = q.gauss_legendre(np.stack([br, 0.5 * br]), npts)
    assert t2.shape == w2.shape == (2, t.size) and np.array_equal(t2[0], t) and np.array_equal(w2[0], w)
    assert (t2[1] > 0.5 * br[0]).all() and (t2[1] < 0.5 * br[-1]).all()
