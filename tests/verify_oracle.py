"""CPU restatement of ntg_batch_verify -- TEST INFRASTRUCTURE (tests/test_verify_oracle.py tests it alone; tests/test_gpu_verify.py
compares the device with it).

The flags come from the oracle's SplineInterp (orc_spline_interp, colloc.c:449-484) at every breakpoint, as tests/test_gpu_cost.py::ref_vals
computes them; the six callbacks from orc_family_* of oracle/liborc.so for the built-in families and from the host shims
(family_oracle.Callbacks, param_oracle.Shim) for modules and the obstacle field.  The definition of include/ntg_amd.h in float64:

    h = 2^-17 max(1, |z_v|), zp = z_v + h, zm = z_v - h, fd = (f(zp) - f(zm)) / (zp - zm)        only entry v moves
    an = df[v] or dc[j][v] at the unperturbed z, scale = max(1, |f(z)|, |an|, |fd|)
    e = |fd - an| / scale  (entries the slot's list names)      l = max(|an|, |fd|) / scale  (entries it does not name)

restate() returns the dense tables e, l [function][breakpoint][entry] of every slot and problem, and err / where / leak / leak_where as
the library defines them: the maximum, on ties the smallest (function * nbps + breakpoint) * nz + entry, a NaN beats every number."""
from __future__ import annotations
import ctypes as C
import os

import numpy as np

import orc
import family_oracle as fo
import param_oracle as po
from ntg_amd import configs as cf
from ntg_amd.spec import Spec

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
SLOTS = ("icf", "ucf", "fcf", "nlicf", "nltcf", "nlfcf")
ICF = C.CFUNCTYPE(None, ip, ip, dp, dp, C.POINTER(dp))
UCF = C.CFUNCTYPE(None, ip, ip, ip, dp, dp, C.POINTER(dp))
NLIC = C.CFUNCTYPE(None, ip, ip, dp, C.POINTER(dp), C.POINTER(dp))
NLTC = C.CFUNCTYPE(None, ip, ip, ip, dp, C.POINTER(dp), C.POINTER(dp))
TYPES = dict(icf=ICF, ucf=UCF, fcf=ICF, nlicf=NLIC, nltcf=NLTC, nlfcf=NLIC)
H0 = 2.0 ** -17


def builtin_callbacks(spec):
    """the oracle's six callbacks of a built-in family (oracle/families.c) as {slot: callable or None}"""
    L = orc.lib()
    out = {}
    for k in SLOTS:
        get = getattr(L, "orc_family_" + k)
        get.restype = C.c_void_p
        get.argtypes = [C.c_int]
        ptr = get(spec.family)
        out[k] = TYPES[k](ptr) if ptr else None
    L.orc_family_set_nout(spec.nout)
    return out


def shim_callbacks(cb):
    """... of a host shim (family_oracle.Callbacks / param_oracle.Shim)"""
    return {k: (TYPES[k](cb.fn[k].value) if cb.fn.get(k) is not None and cb.fn[k].value else None) for k in SLOTS}


def config_W(family: int, ninterv: int = 8, order: int = 6, mult: int = 3, T: float = 4.0) -> Spec:
    """The test plan of the family with planted errors (tests/modules/miswired_family.hpp, loaded as `family`).  Every list names exactly
    the entries its callback reads -- except fcostav, which omits (output 1, deriv 2): planted defect 3."""
    nz = 6
    lic = np.zeros((2, nz)); lic[0, 0] = 1.0; lic[1, 3] = 1.0
    lfc = np.zeros((2, nz)); lfc[0, 0] = 1.0; lfc[1, 3] = 1.0
    return Spec(
        nout=2, bps=cf.linspace_c(0.0, T, 5 * ninterv + 1), kninterv=[ninterv] * 2,
        knots=[cf.linspace_c(0.0, T, ninterv + 1) for _ in range(2)], order=[order] * 2, mult=[mult] * 2, maxderiv=[3] * 2,
        family=family, lic=lic, ltc=np.zeros((0, nz)), lfc=lfc, nnlic=1, nnltc=2, nnlfc=1,
        icav=[(0, 0), (0, 1), (1, 1)], tcav=[(0, 0), (0, 1), (1, 0), (1, 1)], fcav=[(0, 1), (1, 1)],
        nicf=1, nucf=1, nfcf=1, icostav=[(0, 0), (1, 0), (1, 1)], tcostav=[(0, 0), (0, 1), (0, 2), (1, 0), (1, 2)],
        fcostav=[(0, 0), (1, 0)], name=f"W:miswired-k{order}-l{ninterv}")


# where the three defects sit: slot -> (kind, function, flag entry)
PLANTED = {4: ("err", 1, 4), 1: ("err", 0, 2), 2: ("leak", 0, 5)}


def flags(spec, x, knots=None, bps=None):
    """z [batch][nbps][nz]: SplineInterp of every output at every breakpoint.  knots / bps [batch][...]: per-problem grids (every output
    on problem b's knots)"""
    L = orc.lib()
    x = np.asarray(x, dtype=np.float64)
    nb = x.shape[0]
    iC = np.concatenate([[0], np.cumsum(spec.ncoef)])
    iz = np.concatenate([[0], np.cumsum(spec.maxderiv)])
    out = np.zeros((nb, spec.nbps, spec.nz))
    for b in range(nb):
        grid = np.asarray(spec.bps if bps is None else bps[b], dtype=np.float64)
        for o in range(spec.nout):
            kn = np.ascontiguousarray(spec.knots[o] if knots is None else knots[b], dtype=np.float64)
            co = np.ascontiguousarray(x[b, iC[o]:iC[o + 1]])
            zo = np.zeros(int(spec.maxderiv[o]))
            for i in range(spec.nbps):
                L.orc_spline_interp(zo.ctypes.data_as(dp), C.c_double(float(grid[i])), kn.ctypes.data_as(dp), int(spec.kninterv[o]),
                                    co.ctypes.data_as(dp), int(spec.ncoef[o]), int(spec.order[o]), int(spec.mult[o]), int(spec.maxderiv[o]))
                out[b, i, iz[o]:iz[o + 1]] = zo
    return out


class _Caller:
    """one slot's callback on a flat flag: values [nf] and gradients [nf][nz]"""

    def __init__(self, spec, slot, fn, nf):
        self.spec, self.slot, self.fn, self.nf = spec, slot, fn, nf
        self.iz = np.concatenate([[0], np.cumsum(spec.maxderiv)])
        self.z = [np.zeros(int(d)) for d in spec.maxderiv]
        self.zp = (dp * spec.nout)(*[a.ctypes.data_as(dp) for a in self.z])
        self.c = np.zeros(max(nf, 1))
        self.d = np.zeros((max(nf, 1), spec.nz))
        self.dcp = (dp * max(nf, 1))(*[self.d[j].ctypes.data_as(dp) for j in range(max(nf, 1))])
        self.mode, self.ns, self.i = C.c_int(2), C.c_int(0), C.c_int(0)

    def __call__(self, zflat, i):
        for o, a in enumerate(self.z):
            a[:] = zflat[self.iz[o]:self.iz[o + 1]]
        self.mode.value = 2; self.i.value = i
        self.c[:] = 0.0; self.d[:] = 0.0
        k = self.slot
        if k in ("icf", "fcf"):
            self.fn(C.byref(self.mode), C.byref(self.ns), self.c.ctypes.data_as(dp), self.d[0].ctypes.data_as(dp), self.zp)
        elif k == "ucf":
            self.fn(C.byref(self.mode), C.byref(self.ns), C.byref(self.i), self.c.ctypes.data_as(dp), self.d[0].ctypes.data_as(dp), self.zp)
        elif k in ("nlicf", "nlfcf"):
            self.fn(C.byref(self.mode), C.byref(self.ns), self.c.ctypes.data_as(dp), self.dcp, self.zp)
        else:
            self.fn(C.byref(self.mode), C.byref(self.ns), C.byref(self.i), self.c.ctypes.data_as(dp), self.dcp, self.zp)
        return self.c[:self.nf].copy(), self.d[:self.nf].copy()


def _mask(spec, lst):
    iz = np.concatenate([[0], np.cumsum(spec.maxderiv)])
    m = np.zeros(spec.nz, dtype=bool)
    for o, d in lst:
        m[iz[o] + d] = True
    return m


def slot_setup(spec):
    """per slot: (functions, breakpoints audited, named entries [nz])"""
    P = spec.nbps
    return [(spec.nicf and 1, [0], _mask(spec, spec.icostav)), (spec.nucf and 1, list(range(P)), _mask(spec, spec.tcostav)),
            (spec.nfcf and 1, [P - 1], _mask(spec, spec.fcostav)), (spec.nnlic, [0], _mask(spec, spec.icav)),
            (spec.nnltc, list(range(P)), _mask(spec, spec.tcav)), (spec.nnlfc, [P - 1], _mask(spec, spec.fcav))]


def _fmax(*a):
    """max that ignores NaNs (the device's fmax)"""
    a = [v for v in a if v == v]
    return max(a) if a else float("nan")


def point_tables(call, z, i, nf):
    """e, l [nf][nz] of one slot at one point"""
    nz = z.size
    c0, an = call(z, i)
    e = np.zeros((nf, nz)); l = np.zeros((nf, nz))
    for v in range(nz):
        zv = float(z[v])
        h = H0 * _fmax(1.0, abs(zv))
        zp, zm = zv + h, zv - h
        zq = z.copy(); zq[v] = zp
        cp, _ = call(zq, i)
        zq[v] = zm
        cm, _ = call(zq, i)
        for j in range(nf):
            fd = (float(cp[j]) - float(cm[j])) / (zp - zm)
            a = float(an[j, v])
            scale = _fmax(1.0, abs(float(c0[j])), abs(a), abs(fd))
            e[j, v] = abs(fd - a) / scale
            m = float("nan") if (a != a or fd != fd) else max(abs(a), abs(fd))
            l[j, v] = m / scale
    return e, l


def _maximum(tab, sel):
    """(value, [function, breakpoint, entry]) of the library's maximum over the entries sel [nz] of tab [nf][nbps][nz]"""
    if tab.size == 0 or not sel.any():
        return 0.0, [-1, -1, -1]
    t = np.where(sel[None, None, :], tab, 0.0)
    flat = t.ravel()
    nan = np.isnan(flat)
    k = int(np.argmax(nan)) if nan.any() else int(np.argmax(flat))   # the first of equal values: the smallest key
    if not nan.any() and flat[k] == 0.0:
        return 0.0, [-1, -1, -1]
    nf, P, nz = tab.shape
    return float(flat[k]), [k // (P * nz), (k // nz) % P, k % nz]


def restate(spec, x, cbs, knots=None, bps=None, set_problem=None):
    """The audit of x [batch][nC].  cbs: {slot: callable or None}; set_problem(b): called before problem b is evaluated (shims that keep
    one problem's parameters).  Returns dict(err [nb][6], where [nb][6][3], leak, leak_where, e, l) with e / l [nb] lists of six tables
    [nf][nbps][nz] (zero where a slot has no point)."""
    x = np.asarray(x, dtype=np.float64)
    nb, P, nz = x.shape[0], spec.nbps, spec.nz
    Z = flags(spec, x, knots, bps)
    setup = slot_setup(spec)
    out = dict(err=np.zeros((nb, 6)), where=-np.ones((nb, 6, 3), dtype=np.int32), leak=np.zeros((nb, 6)),
               leak_where=-np.ones((nb, 6, 3), dtype=np.int32), e=[], l=[])
    for b in range(nb):
        if set_problem:
            set_problem(b)
        eb, lb = [], []
        for s, (nf, pts, named) in enumerate(setup):
            nf = int(nf)
            e = np.zeros((nf, P, nz)); l = np.zeros((nf, P, nz))
            if nf:
                assert cbs[SLOTS[s]] is not None, "the plan uses slot %s but there is no callback for it" % SLOTS[s]
                call = _Caller(spec, SLOTS[s], cbs[SLOTS[s]], nf)
                for i in pts:
                    e[:, i, :], l[:, i, :] = point_tables(call, Z[b, i], i, nf)
            out["err"][b, s], out["where"][b, s] = _maximum(e, named)
            out["leak"][b, s], out["leak_where"][b, s] = _maximum(l, ~named)
            eb.append(e); lb.append(l)
        out["e"].append(eb); out["l"].append(lb)
    return out


def floor(ref, planted=()):
    """N: the largest err and leak over the clean slots (all but `planted`)"""
    clean = [s for s in range(6) if s not in planted]
    return float(max(np.nanmax(ref["err"][:, clean]), np.nanmax(ref["leak"][:, clean])))


# ---- the cases both test files use: name -> (spec, callbacks, set_problem or None, parameters or None) ----
def builtin_case(spec):
    return spec, builtin_callbacks(spec), None, None


def obstacle_field_case(nb, nobs=3):
    spec = cf.config_OF(nobs, ninterv=4)
    prm, _, _ = cf.obstacle_field_problems(nb, nobs)
    shim = po.Shim("obstacle_field_host")
    return spec, shim_callbacks(shim), (lambda b: shim.set_problem(spec, prm[b])), prm


def tracking_case(family, nb):
    spec = cf.config_TR(family)
    prm, _, _ = cf.tracking_problems(spec, nb)
    shim = po.Shim("tracking_host")
    return spec, shim_callbacks(shim), (lambda b: shim.set_problem(spec, prm[b])), prm


def unicycle_case(family):
    spec = cf.config_U(family)
    return spec, shim_callbacks(fo.Callbacks(fo.build_shim("unicycle_host"), "uni_")), None, None


def miswired_case(family):
    spec = config_W(family)
    return spec, shim_callbacks(fo.Callbacks(fo.build_shim("miswired_host"), "mw_")), None, None
