"""The reference's example programs (vanderpol, kincar) at the drop-in boundary, self-contained:
tests/drivers/dropin_drv.c makes the examples' call sequence on their problem data, written against
include/ntg.h.

CPU suite: link that driver against the oracle's ABI library and check the optima the examples print
(this pins the oracle on the only executable tests the reference has), and link it against
libntg_amd.so (the product; it needs a GPU to run, tests/test_gpu_dropin.py runs it there).  Run with
"files", the driver also calls the examples' remaining helpers (PrintVector, PrintMatrix, FreeDoubleMatrix).
"""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "tests", "drivers", "dropin_drv.c")
# what each example program calls from include/ntg.h
EXAMPLE_SYMBOLS = {"vanderpol": ("ntg", "npsoloption", "linspace", "PrintVector", "DoubleMatrix", "FreeDoubleMatrix"),
                   "kincar": ("ntg", "npsoloption", "linspace", "PrintVector", "DoubleMatrix", "FreeDoubleMatrix",
                              "SplineInterp", "MakeMatrix", "PrintMatrix")}


def build(tmp_path, libdir, lib, extra=()):
    exe = tmp_path / ("dropin_drv_" + lib)
    subprocess.check_call(["gcc", "-O1", "-w", "-I", os.path.join(ROOT, "include"), DRV, "-o", str(exe), "-L", libdir, "-l" + lib, "-lm",
                           "-Wl,-rpath," + libdir] + list(extra))
    return exe


def run_oracle(tmp_path, which):
    import orc
    orc.build()
    exe = build(tmp_path, os.path.join(ROOT, "oracle"), "orc_ntg")
    out = subprocess.run([str(exe), which, "files"], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
    res = np.array([l.split()[1:] for l in out.splitlines() if l.startswith("RESULT")][0], dtype=float)
    return int(res[0]), res[1], res[2:]


@pytest.mark.parametrize("name", ["vanderpol", "kincar"])
def test_examples_link_against_the_product_library(tmp_path, name):
    """a program written against include/ntg.h that calls every helper the example program calls LINKS against libntg_amd.so (the
    product; it needs a GPU to run, so this container only links), and the library exports each of those symbols"""
    lib = os.path.join(ROOT, "ntg_amd", "libntg_amd.so")
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    exe = build(tmp_path, os.path.join(ROOT, "ntg_amd"), "ntg_amd", ["-Wl,--no-undefined"])
    und = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    und = {l.split()[-1].split("@")[0] for l in und.splitlines() if l.split()}
    for sym in EXAMPLE_SYMBOLS[name]:
        assert sym in und, sym
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1].split("@")[0] for l in exported.splitlines() if len(l.split()) >= 3 and l.split()[1] in "TWiV"}
    for sym in EXAMPLE_SYMBOLS[name]:
        assert sym in exported, sym


def test_vanderpol_example_optimum(tmp_path):
    inform, obj, coef = run_oracle(tmp_path, "vanderpol")
    assert inform == 0
    assert abs(obj - 1.7022142628309958) < 1e-9
    np.testing.assert_allclose(coef, [1, 1, 0.39374, -0.036958, -0.439532, -0.716865, -0.244974], atol=2e-6)
    np.testing.assert_allclose(np.loadtxt(tmp_path / "coef1"), coef, rtol=1e-5, atol=1e-12)   # PrintVector("coef1"), %g


def test_kincar_example_optimum(tmp_path):
    inform, obj, coef = run_oracle(tmp_path, "kincar")
    assert inform == 0
    assert abs(obj - 2.457581141950512) < 1e-9
    assert np.array_equal(np.loadtxt(tmp_path / "lic"), np.eye(6))                            # PrintMatrix("lic")
    # the example's printed trajectory: 30 times on [0, 5], both flat outputs (x, y) through SplineInterp, speed from their derivatives
    # (order 5, multiplicity 3, 2 intervals per output: the driver's kincar shape)
    spl = C.CDLL(os.path.join(ROOT, "oracle", "liborc_ntg.so")).SplineInterp
    dp = C.POINTER(C.c_double)
    spl.argtypes = [dp, C.c_double, dp, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int]
    knots = np.linspace(0.0, 5.0, 3)
    cf = np.ascontiguousarray(coef.reshape(2, 7))
    traj = np.zeros((30, 4))                                   # time x y v
    for i, t in enumerate(5.0 * np.arange(30) / 29):
        fz = np.zeros((2, 3))
        for j in range(2):
            spl(fz[j].ctypes.data_as(dp), t, knots.ctypes.data_as(dp), 2, cf[j].ctypes.data_as(dp), 7, 5, 3, 3)
        traj[i] = t, fz[0, 0], fz[1, 0], np.hypot(fz[0, 1], fz[1, 1])
    np.testing.assert_allclose(traj[0, 1:3], [0, -2], atol=1e-3)
    np.testing.assert_allclose(traj[-1, 1:3], [40, 2], atol=1e-3)
    np.testing.assert_allclose(traj[:, 3], 8.0, atol=0.25)    # speed stays near 8 m/s
