"""CPU oracle for a family given as host callbacks (a shim compiled from a module's family header, e.g. tests/modules/
unicycle_host.cpp): builds one orc_problem per problem through orc_problem_make of oracle/liborc.so and calls orc_funobj /
orc_funcon / orc_sqp_solve -- TEST INFRASTRUCTURE (tests/orc.py is the binding of the built-in families)."""
from __future__ import annotations
import ctypes as C
import os
import subprocess
import numpy as np

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


def build_shim(name: str) -> str:
    """tests/modules/<name>.cpp -> .so (plain g++, -ffp-contract=off like the oracle), rebuilt when older than its inputs"""
    src = os.path.join(HERE, "modules", name + ".cpp")
    so = os.path.join(HERE, "modules", name + ".so")
    deps = [src, os.path.join(ROOT, "include", "ntg_amd_family.hpp")] + \
        [os.path.join(ROOT, "ntg_amd", "modules", f) for f in os.listdir(os.path.join(ROOT, "ntg_amd", "modules")) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               "-o", so, src])
    return so


class Callbacks:
    """the six callbacks of a shim, by symbol prefix (missing ones are NULL)"""

    def __init__(self, so: str, prefix: str):
        self.lib = C.CDLL(so)
        self.fn = {}
        for k in ("icf", "ucf", "fcf", "nlicf", "nltcf", "nlfcf"):
            self.fn[k] = C.cast(getattr(self.lib, prefix + k), C.c_void_p) if hasattr(self.lib, prefix + k) else None


def _setup():
    L = orc.lib()
    L.orc_problem_make.restype = C.c_void_p
    L.orc_problem_free.argtypes = [C.c_void_p]
    L.orc_funobj.argtypes = [C.c_void_p, ip, dp, dp, dp, ip]
    L.orc_funcon.argtypes = [C.c_void_p, ip, dp, dp, dp, ip]
    L.orc_sqp_solve.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L


class Problem:
    """one orc_problem of `spec` with the shim's callbacks and the bounds (lower, upper) [nbounds]"""

    def __init__(self, spec, cb: Callbacks, lower, upper):
        L = self.L = _setup()
        k = self._keep = {}
        k["bps"] = np.ascontiguousarray(spec.bps, dtype=np.float64)
        for nm in ("kninterv", "order", "mult", "maxderiv"):
            k[nm] = np.asarray(getattr(spec, nm), dtype=np.int32)
        k["knots"] = [np.ascontiguousarray(x, dtype=np.float64) for x in spec.knots]
        k["kp"] = (dp * spec.nout)(*[x.ctypes.data_as(dp) for x in k["knots"]])

        def rows(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            k.setdefault("rows", []).append(a)
            return (dp * max(a.shape[0], 1))(*[a[i].ctypes.data_as(dp) for i in range(a.shape[0])])

        def avs(lst):
            arr = (orc.AVc * max(len(lst), 1))()
            for j, (o, d) in enumerate(lst):
                arr[j].output, arr[j].deriv = o, d
            k.setdefault("avs", []).append(arr)
            return arr
        k["lo"] = np.ascontiguousarray(lower, dtype=np.float64); k["up"] = np.ascontiguousarray(upper, dtype=np.float64)
        f = cb.fn
        self.p = L.orc_problem_make(
            spec.nout, k["bps"].ctypes.data_as(dp), spec.nbps, k["kninterv"].ctypes.data_as(ip), k["kp"], k["order"].ctypes.data_as(ip),
            k["mult"].ctypes.data_as(ip), k["maxderiv"].ctypes.data_as(ip),
            spec.nlic, rows(spec.lic), spec.nltc, rows(spec.ltc), spec.nlfc, rows(spec.lfc),
            spec.nnlic, f["nlicf"], spec.nnltc, f["nltcf"], spec.nnlfc, f["nlfcf"],
            len(spec.icav), avs(spec.icav), len(spec.tcav), avs(spec.tcav), len(spec.fcav), avs(spec.fcav),
            k["lo"].ctypes.data_as(dp), k["up"].ctypes.data_as(dp),
            spec.nicf, f["icf"], spec.nucf, f["ucf"], spec.nfcf, f["fcf"],
            len(spec.icostav), avs(spec.icostav), len(spec.tcostav), avs(spec.tcostav), len(spec.fcostav), avs(spec.fcostav))
        self.spec = spec

    def close(self):
        if self.p:
            self.L.orc_problem_free(self.p)
            self.p = None

    def __del__(self):
        self.close()

    def eval(self, x, mode=2):
        """f, g, c [ncnln] and the dense Jacobian [ncnln, nC] at x"""
        sp = self.spec
        x = np.ascontiguousarray(x, dtype=np.float64)
        f = np.zeros(1); g = np.zeros(sp.nC); c = np.zeros(max(sp.ncnln, 1)); J = np.zeros((sp.nC, max(sp.ncnln, 1)))
        md = C.c_int(mode); ns = C.c_int(1)
        self.L.orc_funobj(self.p, C.byref(md), x.ctypes.data_as(dp), f.ctypes.data_as(dp), g.ctypes.data_as(dp), C.byref(ns))
        md = C.c_int(mode)
        self.L.orc_funcon(self.p, C.byref(md), x.ctypes.data_as(dp), c.ctypes.data_as(dp), J.ctypes.data_as(dp), C.byref(ns))
        Jm = J[:, :sp.ncnln].T.copy()   # column-major ncnln x nC, the reference layout (GcJac starts zeroed, ntg.c:217)
        return dict(f=f[0], g=g, c=c[:sp.ncnln], cJac=Jm)

    def solve(self, x0, opts):
        x = np.array(x0, dtype=np.float64, copy=True)
        res = orc.Result()
        self.L.orc_sqp_solve(self.p, x.ctypes.data_as(dp), C.byref(opts), C.byref(res), None, None, None, None, 0)
        return dict(x=x, objective=res.objective, inform=res.inform, iters=res.iters, nfev=res.nfev)


def solve_batch(spec, cb, lower, upper, x0, opts):
    out = dict(x=np.zeros_like(np.asarray(x0, dtype=np.float64)), objective=np.zeros(len(x0)), inform=np.zeros(len(x0), dtype=np.int32),
               iters=np.zeros(len(x0), dtype=np.int32), nfev=np.zeros(len(x0), dtype=np.int32))
    for b in range(len(x0)):
        pr = Problem(spec, cb, lower[b], upper[b])
        r = pr.solve(x0[b], opts)
        pr.close()
        for key in out:
            out[key][b] = r[key]
    return out
