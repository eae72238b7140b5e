"""Per-problem family parameters (ntg_plan_set_params) -- what can be checked without a GPU: the new C entry points are exported, the
tracking module declares its parameters, the obstacle-field family's arithmetic (ntg_amd/csrc/obstacle_field.hpp, compiled for the host
through the oracle's shim) agrees with finite differences and with its dense form, and the new kernels pass the call-boundary audit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import param_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = os.path.join(ROOT, "ntg_amd", "modules")
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return family.build_module(os.path.join(MODULES, "tracking.hip"))


@pytest.fixture(scope="module")
def shim():
    L = C.CDLL(po.build_shim("obstacle_field_host"))
    L.of_val.argtypes = [C.c_int, dp, dp, dp]
    L.of_vjp.argtypes = [C.c_int, dp, dp, dp, dp]
    L.of_dense.argtypes = [C.c_int, dp, dp, dp, dp]
    L.of_block.argtypes = [C.c_int, dp, dp, C.c_double, C.c_int, dp, dp]
    return L


def _p(a):
    return a.ctypes.data_as(dp)


def test_param_entry_points_exported(built):
    from ntg_amd import build
    syms = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ("ntg_plan_param_count", "ntg_plan_set_params", "ntg_plan_clear_params"):
        assert " " + name + "\n" in syms, name


class _Desc(C.Structure):
    """ntg_family_module_desc of ntg_amd/csrc/family_module.hpp"""
    _fields_ = [("abi", C.c_ulonglong)] + [(n, C.c_int) for n in ("s_dims", "s_tables", "s_layout", "s_params", "s_eval", "s_sqp")] + \
        [("name", C.c_char_p), ("dm", C.c_int), ("nnlic", C.c_int), ("nnltc", C.c_int), ("nnlfc", C.c_int), ("nout", C.c_int),
         ("launch_eval", C.c_void_p), ("launch_sqp", C.c_void_p), ("nparam", C.c_int), ("nparam_bp", C.c_int)]


def _descriptor(so):
    lib = C.CDLL(so, mode=os.RTLD_LOCAL)
    lib.ntg_family_module_v1.restype = C.POINTER(_Desc)
    return lib.ntg_family_module_v1().contents


def test_tracking_module_declares_breakpoint_parameters(built):
    from ntg_amd import api, build
    d = _descriptor(built)
    assert d.name == b"tracking" and (d.nparam, d.nparam_bp) == (0, 2) and d.nout == 2
    assert d.abi == int(build.abi_stamp()[:-3], 16)
    fam = api.load_family(built)
    assert api.family_info(fam) == dict(name="tracking", maxderiv=3, nnlic=0, nnltc=0, nnlfc=0, nout=2)


@pytest.mark.parametrize("name", ["unicycle", "testfam_module"])
def test_modules_without_parameters_declare_none(built, name):
    from ntg_amd import family
    d = _descriptor(family.build_module(os.path.join(MODULES, name + ".hip")))
    assert (d.nparam, d.nparam_bp) == (0, 0)


def _field(m, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=6) * 3.0
    prm = rng.normal(size=2 * m) * 3.0
    t = rng.normal(size=m)
    return z, prm, t


@pytest.mark.parametrize("m", [1, 3, 8])
def test_field_rows_match_finite_differences_and_dense_form(shim, m):
    z, prm, t = _field(m, 7 + m)
    c = np.zeros(m); cd = np.zeros(m); dc = np.zeros((m, 6))
    shim.of_val(m, _p(z), _p(prm), _p(c))
    shim.of_dense(m, _p(z), _p(prm), _p(cd), _p(dc))
    assert np.array_equal(c, cd)
    cx, cy = prm[0::2], prm[1::2]
    assert np.allclose(c, (z[0] - cx) ** 2 + (z[3] - cy) ** 2, rtol=1e-14)
    h = 1e-6
    for v in range(6):
        zp, zm = z.copy(), z.copy(); zp[v] += h; zm[v] -= h
        cp, cm = np.zeros(m), np.zeros(m)
        shim.of_val(m, _p(zp), _p(prm), _p(cp)); shim.of_val(m, _p(zm), _p(prm), _p(cm))
        assert np.allclose(dc[:, v], (cp - cm) / (2 * h), rtol=1e-7, atol=1e-7)
    # vjp: df += J' t, on top of what df holds
    df0 = np.arange(6.0)
    df = df0.copy()
    shim.of_vjp(m, _p(z), _p(t), _p(prm), _p(df))
    assert np.allclose(df - df0, dc.T @ t, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("m", [1, 4, 8])
@pytest.mark.parametrize("curv", [0, 1])
def test_field_block_is_gauss_newton_plus_curvature(shim, m, curv):
    z, prm, t = _field(m, 31 + m)
    t[m // 2] = 0.0   # an inactive row contributes no Gauss-Newton term
    mu = 0.7
    B = np.zeros(4)
    shim.of_block(m, _p(z), _p(t), mu, curv, _p(prm), _p(B))
    B = B.reshape(2, 2)

    def phi(x, y):   # sum_j t_j c_j on the (x, y) entries
        return sum(t[j] * ((x - prm[2 * j]) ** 2 + (y - prm[2 * j + 1]) ** 2) for j in range(m))
    h = 1e-4
    x, y = z[0], z[3]
    H = np.array([[(phi(x + h, y) - 2 * phi(x, y) + phi(x - h, y)) / h ** 2,
                   (phi(x + h, y + h) - phi(x + h, y - h) - phi(x - h, y + h) + phi(x - h, y - h)) / (4 * h * h)],
                  [0.0, (phi(x, y + h) - 2 * phi(x, y) + phi(x, y - h)) / h ** 2]])
    H[1, 0] = H[0, 1]
    want = curv * H
    for j in range(m):
        if t[j] != 0.0:
            a = 2.0 * np.array([x - prm[2 * j], y - prm[2 * j + 1]])
            want = want + mu * np.outer(a, a)
    assert np.allclose(B, want, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(want).max()))


def test_field_and_tracking_kernels_pass_audits(built):
    from ntg_amd import call_audit, family, isa_audit
    asm = os.path.join(ROOT, "ntg_amd", "csrc", "fam_obstacle_field-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(asm)
    assert call_audit.audit(asm) == []
    text = open(asm, errors="replace").read()
    assert "_Z10sqp_kernelILi6E" in text and "_Z11eval_kernelILi6E" in text   # the field family's own instances
    tasm = family.assembly_path(os.path.join(MODULES, "tracking.hip"))
    assert os.path.exists(tasm) and call_audit.audit(tasm) == []
    # the assembly rules of the hand-tuned kernels (no compiler use of the accumulator registers they reserve, no spills there) hold too
    for path in (asm, tasm):
        assert isa_audit.audit("hipcc", "", "", [], 0, asm_path=path) == [], path
