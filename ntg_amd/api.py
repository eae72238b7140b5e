"""ctypes binding of libntg_amd.so (include/ntg_amd.h).  Host plumbing only: it marshals a Spec
into the C ABI and passes torch device pointers; all numerics run in the library's HIP kernels.
There is no fallback: if the library is missing or no GPU is visible, calls raise."""
from __future__ import annotations
import ctypes as C
import os
from typing import Optional
import numpy as np

from .spec import Spec

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NTG_AMD_LIB") or os.path.join(_HERE, "libntg_amd.so")   # NTG_AMD_LIB: a tuning build of the same library (tests/tools_variants.py)
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


class NtgError(RuntimeError):
    pass


class _AV(C.Structure):
    _fields_ = [("output", C.c_int), ("deriv", C.c_int)]


class _Spec(C.Structure):
    _fields_ = [("nout", C.c_int), ("nbps", C.c_int), ("bps", dp), ("kninterv", ip),
                ("knots", C.POINTER(dp)), ("order", ip), ("mult", ip), ("maxderiv", ip),
                ("family", C.c_int),
                ("nlic", C.c_int), ("nltc", C.c_int), ("nlfc", C.c_int),
                ("lic", dp), ("ltc", dp), ("lfc", dp),
                ("nnlic", C.c_int), ("nnltc", C.c_int), ("nnlfc", C.c_int),
                ("nicav", C.c_int), ("ntcav", C.c_int), ("nfcav", C.c_int),
                ("icav", C.POINTER(_AV)), ("tcav", C.POINTER(_AV)), ("fcav", C.POINTER(_AV)),
                ("nicf", C.c_int), ("nucf", C.c_int), ("nfcf", C.c_int),
                ("nicostav", C.c_int), ("ntcostav", C.c_int), ("nfcostav", C.c_int),
                ("icostav", C.POINTER(_AV)), ("tcostav", C.POINTER(_AV)), ("fcostav", C.POINTER(_AV)),
                ("lin_ineq", ip)]


class SolveOpts(C.Structure):
    _fields_ = [("itlim", C.c_int), ("opttol", C.c_double), ("steplimit", C.c_double),
                ("ls_mu", C.c_double), ("ls_eta", C.c_double), ("ls_maxfev", C.c_int),
                ("hessian", C.c_int), ("fixed_iters", C.c_int), ("block_threads", C.c_int), ("qn_memory", C.c_int), ("warm_start", C.c_int)]


class FormTerm(C.Structure):
    """ntg_form_term: w (z[u] - a)(z[v] - b), or w (z[u] - a) when v == -1; a = su + fprm[pu], b = sv + fprm[pv] (index -1: no parameter)"""
    _fields_ = [("u", C.c_int), ("v", C.c_int), ("pu", C.c_int), ("pv", C.c_int), ("w", C.c_double), ("su", C.c_double), ("sv", C.c_double)]


class Ratio(C.Structure):
    """ntg_ratio: the product of the forms num[:nnum] over the product of the forms den[:nden]; an empty side is 1"""
    _fields_ = [("nnum", C.c_int), ("nden", C.c_int), ("num", C.c_int * 4), ("den", C.c_int * 4)]


class TrigTerm(C.Structure):
    """ntg_trig_term: w g(theta), theta = sum_i coef[i] z[ent[i]] + phase + fprm[pp] (index -1: no parameter); g = sin, cos or the identity by kind"""
    _fields_ = [("kind", C.c_int), ("nent", C.c_int), ("pp", C.c_int), ("pad", C.c_int), ("ent", C.c_int * 4), ("coef", C.c_double * 4), ("phase", C.c_double), ("w", C.c_double)]


TRIG_MAXFORMS, TRIG_MAXTERMS, TRIG_MAXENT = 8, 4, 4   # NTG_TRIG_*
TRIG_SIN, TRIG_COS, TRIG_LIN = 0, 1, 2



class MinmaxMember(C.Structure):
    """ntg_minmax_member: q_form(z) + c + fprm[pc] (index -1: no parameter)"""
    _fields_ = [("form", C.c_int), ("pc", C.c_int), ("c", C.c_double)]


class MinmaxGroup(C.Structure):
    """ntg_minmax_group: OUTER over nclause clauses of INNER over nmem[k] members each, outer / inner = MINMAX_MIN or MINMAX_MAX"""
    _fields_ = [("outer", C.c_int), ("inner", C.c_int), ("nclause", C.c_int), ("pad", C.c_int), ("nmem", C.c_int * 8)]


MINMAX_MIN, MINMAX_MAX = 0, 1
MINMAX_MAXFORMS, MINMAX_MAXTERMS, MINMAX_MAXGROUPS, MINMAX_MAXCLAUSES, MINMAX_MAXMEMBERS = 16, 40, 4, 8, 16   # NTG_MINMAX_*

_lib = None


def lib():
    """Load libntg_amd.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NtgError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.ntg_last_error.restype = C.c_char_p
        L.ntg_solve_kernel_name.restype = C.c_char_p
        L.ntg_batch_solve_kernel.restype = C.c_char_p
        L.ntg_batch_solve_kernel.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ntg_batch_workspace_bytes.restype = C.c_longlong
        L.ntg_batch_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ntg_plan_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ntg_plan_destroy.argtypes = [C.c_void_p]
        L.ntg_plan_dims.argtypes = [C.c_void_p] + [ip] * 7
        L.ntg_plan_tables.argtypes = [C.c_void_p, dp, ip, dp]
        L.ntg_plan_grid_tables.argtypes = [C.c_void_p, C.c_int, dp, ip, dp]
        L.ntg_batch_bounds.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.ntg_batch_eval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.ntg_batch_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_longlong, C.c_void_p]
        L.ntg_basis_batch.argtypes = [C.c_int] * 6 + [C.c_void_p] * 5
        L.ntg_batch_mpc_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_longlong, C.c_void_p]
        L.ntg_batch_mpc_shift_multipliers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.ntg_batch_interp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_batch_interp_strided.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        L.ntg_batch_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_batch_kkt.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.ntg_batch_cost.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_batch_verify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_batch_envelope.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
        L.ntg_batch_envelope_sos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.ntg_plan_sos_rows.argtypes = [C.c_void_p, ip]
        L.ntg_batch_extrema.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
        L.ntg_plan_extrema_rows.argtypes = [C.c_void_p, ip]
        L.ntg_batch_separation.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 6
        L.ntg_batch_forms.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(FormTerm), C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
        L.ntg_batch_ratios.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(FormTerm), C.c_int, C.c_void_p, C.c_int, C.POINTER(Ratio), C.c_double, C.c_int,
                                       C.c_int] + [C.c_void_p] * 9
        L.ntg_batch_trig.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(TrigTerm), C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 9
        L.ntg_batch_minmax.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, C.POINTER(FormTerm), C.c_int, C.c_void_p, C.c_int, C.POINTER(MinmaxGroup), C.POINTER(MinmaxMember),
                                       C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 10
        L.ntg_batch_refine.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_plan_set_grids.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ntg_plan_clear_grids.argtypes = [C.c_void_p]
        L.ntg_plan_param_count.argtypes = [C.c_void_p, ip]
        L.ntg_plan_set_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ntg_plan_clear_params.argtypes = [C.c_void_p]
        L.ntg_plan_clear_grids.restype = None
        L.ntg_batch_kincar_reverse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.ntg_batch_mpc_shift.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ntg_family_load.argtypes = [C.c_char_p, ip]
        L.ntg_family_info.argtypes = [C.c_int, C.c_char_p, C.c_int] + [ip] * 5
        _lib = L
    return _lib


def _check_tensor(t, dev, dtype=None):
    """the C ABI takes raw device pointers: a tensor of the wrong dtype / device / layout would corrupt memory silently"""
    import torch
    if t is None:
        return
    want = dtype if dtype is not None else torch.float64
    if not (t.is_cuda and t.device == dev and t.dtype == want and t.is_contiguous()):
        raise NtgError(f"tensor must be a contiguous {want} tensor on {dev}, got {t.dtype} on {t.device} (contiguous: {t.is_contiguous()})")


def _check(rc):
    if rc != 0:
        raise NtgError(f"libntg_amd error {rc}: {lib().ntg_last_error().decode()}")


def default_opts(**kw) -> SolveOpts:
    o = SolveOpts()
    lib().ntg_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bisect_out(batch, rows, dev, bounds):
    """the outputs of extrema, forms and ratios for (batch, rows): ext, when, status, npieces and, with bounds, viol and where.  (No row gets one
    row of storage: the library refuses or returns before it writes, and an empty tensor would arrive as a null pointer)"""
    import torch
    rows = max(rows, 1)
    out = {"ext": torch.empty((batch, rows, 4), dtype=torch.float64, device=dev), "when": torch.empty((batch, rows, 2), dtype=torch.float64, device=dev),
           "status": torch.empty((batch, rows), dtype=torch.int32, device=dev), "npieces": torch.empty((batch, rows), dtype=torch.int32, device=dev)}
    if bounds:
        out["viol"] = torch.zeros((batch, 2), dtype=torch.float64, device=dev); out["where"] = torch.full((batch, 2), -1, dtype=torch.int32, device=dev)
    return out


def _declare_forms(forms, fprm, lower, upper, dev, batch, nrows, what, ratios=()):
    """what forms and ratios ask of fprm [batch, nfp], the bounds [batch, nrows] of `what` and the ratios' factor counts, in that order, and
    then the declaration as the library takes it: -> (form_nterms, terms, nfp)"""
    _check_tensor(fprm, dev); _check_tensor(lower, dev); _check_tensor(upper, dev)
    forms = [list(f) for f in forms]
    if (lower is None) != (upper is None):
        raise NtgError("pass both bounds or neither")
    if lower is not None and (lower.shape != (batch, nrows) or upper.shape != (batch, nrows)):
        raise NtgError(f"the {what}' bounds must be [{batch}, {nrows}]")
    if fprm is not None and (fprm.dim() != 2 or fprm.shape[0] != batch):
        raise NtgError(f"fprm must be [{batch}, nfp]")
    for r, (n, d) in enumerate(ratios):
        if len(n) > RATIO_MAXFACTORS or len(d) > RATIO_MAXFACTORS:
            raise NtgError(f"ratio {r}: nnum and nden must lie in 0 .. {RATIO_MAXFACTORS}")
    nterms = (C.c_int * max(len(forms), 1))(*[len(f) for f in forms])
    flat = [FormTerm(*t) for f in forms for t in f]
    return nterms, (FormTerm * max(len(flat), 1))(*flat), 0 if fprm is None else int(fprm.shape[1])


class Plan:
    """Device-resident, batch-shared part of a problem (ntg_plan)."""

    def __init__(self, spec: Spec, device: int = 0):
        self.spec = spec
        self.device = device
        self.grid_batch = 0   # batch of the per-problem grids in force (set_grids / clear_grids)
        self.param_batch = 0  # batch of the per-problem parameters in force (set_params / clear_params)
        k = self._keep = {}
        k["bps"] = np.ascontiguousarray(spec.bps, dtype=np.float64)
        for nm in ("kninterv", "order", "mult", "maxderiv"):
            k[nm] = np.asarray(getattr(spec, nm), dtype=np.int32)
        k["knots"] = [np.ascontiguousarray(x, dtype=np.float64) for x in spec.knots]
        k["kp"] = (dp * spec.nout)(*[x.ctypes.data_as(dp) for x in k["knots"]])
        for nm in ("lic", "ltc", "lfc"):
            k[nm] = np.ascontiguousarray(getattr(spec, nm), dtype=np.float64).reshape(-1)

        def avs(lst):
            arr = (_AV * max(len(lst), 1))()
            for j, (o, d) in enumerate(lst):
                arr[j].output, arr[j].deriv = o, d
            return arr
        for nm in ("icav", "tcav", "fcav", "icostav", "tcostav", "fcostav"):
            k[nm] = avs(list(getattr(spec, nm)))
        s = _Spec()
        s.nout, s.nbps = spec.nout, spec.nbps
        s.bps = k["bps"].ctypes.data_as(dp)
        s.kninterv = k["kninterv"].ctypes.data_as(ip); s.order = k["order"].ctypes.data_as(ip)
        s.mult = k["mult"].ctypes.data_as(ip); s.maxderiv = k["maxderiv"].ctypes.data_as(ip)
        s.knots = k["kp"]; s.family = spec.family
        s.nlic, s.nltc, s.nlfc = spec.nlic, spec.nltc, spec.nlfc
        s.lic, s.ltc, s.lfc = (k[nm].ctypes.data_as(dp) for nm in ("lic", "ltc", "lfc"))
        s.nnlic, s.nnltc, s.nnlfc = spec.nnlic, spec.nnltc, spec.nnlfc
        s.nicav, s.ntcav, s.nfcav = len(spec.icav), len(spec.tcav), len(spec.fcav)
        s.icav, s.tcav, s.fcav = k["icav"], k["tcav"], k["fcav"]
        s.nicf, s.nucf, s.nfcf = spec.nicf, spec.nucf, spec.nfcf
        s.nicostav, s.ntcostav, s.nfcostav = len(spec.icostav), len(spec.tcostav), len(spec.fcostav)
        s.icostav, s.tcostav, s.fcostav = k["icostav"], k["tcostav"], k["fcostav"]
        if len(spec.lin_ineq):
            assert len(spec.lin_ineq) == spec.nlic + spec.nltc + spec.nlfc
            k["lin_ineq"] = np.asarray(spec.lin_ineq, dtype=np.int32)
            s.lin_ineq = k["lin_ineq"].ctypes.data_as(ip)
        self._cspec = s
        h = C.c_void_p()
        _check(lib().ntg_plan_create(C.byref(s), device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().ntg_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup tables (host copies) ----
    def _host_tables(self, fill):
        """blk, off and A [nclin, nC] as fill(blk, off, A) -- ntg_plan_tables or ntg_plan_grid_tables -- writes them"""
        sp = self.spec
        nblk = sum(sp.nbps * k * d for k, d in zip(sp.order, sp.maxderiv))
        blk = np.zeros(nblk); off = np.zeros((sp.nout, sp.nbps), dtype=np.int32)
        A = np.zeros((sp.nC, max(sp.nclin, 1)))
        _check(fill(blk.ctypes.data_as(dp), off.ctypes.data_as(ip), A.ctypes.data_as(dp)))
        return dict(blk=blk, off=off, A=(A.T.copy() if sp.nclin else np.zeros((0, sp.nC))))

    def tables(self):
        return self._host_tables(lambda *out: lib().ntg_plan_tables(self.h, *out))

    def grid_tables(self, b: int):
        """tables() of problem b's grid after set_grids: its basis blocks, the plan's offsets, and A [nclin, nC] with the equality and
        inequality rows the solver reads for that problem.  Raises without per-problem grids or for b outside [0, batch)."""
        return self._host_tables(lambda *out: lib().ntg_plan_grid_tables(self.h, int(b), *out))

    # ---- batched entry points; tensors are torch CUDA(HIP) float64/int32, contiguous ----
    def bounds(self, lower, upper):
        import torch
        sp = self.spec
        batch = lower.shape[0]
        ntot = sp.nC + sp.nclin + sp.ncnln
        bl = torch.empty((batch, ntot), dtype=torch.float64, device=lower.device); bu = torch.empty_like(bl)
        _check(lib().ntg_batch_bounds(self.h, batch, _ptr(lower), _ptr(upper), _ptr(bl), _ptr(bu), self._stream()))
        return bl, bu

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def eval(self, x, mode: int = 2, want_dense_jac: bool = False, out=None):
        """funobj + funcon for a batch.  `out` (a dict returned by an earlier call with the same shapes) reuses its buffers."""
        import torch
        sp = self.spec
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        batch = x.shape[0]
        dev = x.device
        if out is not None:
            f, g, c, jb = out["f"], out["g"], out.get("c"), out.get("jband")
            cj = out.get("_cj")   # the [batch][nC][ncnln] buffer behind an earlier dense Jacobian, reused
            if want_dense_jac and sp.ncnln and cj is None:
                cj = torch.empty((batch, sp.nC, sp.ncnln), dtype=torch.float64, device=dev)
            for t in (f, g, c, jb):
                _check_tensor(t, dev)
        else:
            f = torch.empty(batch, dtype=torch.float64, device=dev)
            g = torch.empty((batch, sp.nC), dtype=torch.float64, device=dev)
            c = jb = cj = None
            if sp.ncnln:
                c = torch.zeros((batch, sp.ncnln), dtype=torch.float64, device=dev)
                jb = torch.zeros((batch, sp.ncnln, sp.sumk), dtype=torch.float64, device=dev)
                if want_dense_jac:
                    cj = torch.empty((batch, sp.nC, sp.ncnln), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_eval(self.h, batch, _ptr(x), mode, _ptr(f), _ptr(g), _ptr(c), _ptr(jb), _ptr(cj), self._stream()))
        out = dict(f=f, g=g)
        if sp.ncnln:
            out.update(c=c, jband=jb)
            if want_dense_jac:
                out["cJac"] = cj.transpose(1, 2).contiguous()
                out["_cj"] = cj
        return out

    def interp(self, x, times):
        """Flat flag of every problem at the given times: x [batch, nC], times [ntimes] -> [batch, ntimes, nz].
        After set_grids: times [batch, ntimes], every problem at its own times on its own knots."""
        import torch
        _check_tensor(x, x.device)
        if not (times.is_cuda and times.dtype == torch.float64):
            raise NtgError("times must be a float64 tensor on the plan's device")
        batch = x.shape[0]
        stride = self._times_stride(batch, times)
        ntimes = times.shape[-1]
        z = torch.empty((batch, ntimes, self.spec.nz), dtype=torch.float64, device=x.device)
        _check(lib().ntg_batch_interp_strided(self.h, batch, _ptr(x), ntimes, _ptr(times.contiguous()), stride, _ptr(z), self._stream()))
        return z

    def _times_stride(self, batch, times):
        """layout of a time argument: [ntimes] shared by the batch (stride 0) or, after set_grids, [batch, ntimes]"""
        if times.dim() == 1:
            return 0                         # one time vector for the batch (with per-problem grids: every problem on its own knots)
        if times.dim() == 2 and self.grid_batch and times.shape[0] == batch:
            return times.shape[1]
        if times.dim() == 2:
            raise NtgError("per-problem times [batch, ntimes] need per-problem grids of that batch (set_grids); pass a 1-D time vector")
        raise NtgError("times must be [ntimes] or, after set_grids, [batch, ntimes]")

    def check(self, x, lower, upper, times, want_rows: bool = False):
        """The trajectory rows of solved problems BETWEEN the breakpoints (ntg_batch_check): x [batch, nC], bounds [batch, nbounds],
        times [ntimes] or, after set_grids, [batch, ntimes].  Returns dict(viol [batch], where [batch, 2] = (row, time index) of the
        largest violation or (-1, -1)[, rows [batch, nltc + nnltc, ntimes]]); linear trajectory rows come first."""
        import torch
        sp = self.spec
        dev = x.device
        _check_tensor(x, dev); _check_tensor(lower, dev); _check_tensor(upper, dev)
        batch = x.shape[0]
        if not (times.is_cuda and times.dtype == torch.float64):
            raise NtgError("times must be a float64 tensor on the plan's device")
        if lower.shape != (batch, sp.nbounds) or upper.shape != (batch, sp.nbounds):
            raise NtgError(f"bounds must be [{batch}, {sp.nbounds}]")
        stride = self._times_stride(batch, times)
        ntimes = times.shape[-1]
        out = dict(viol=torch.zeros(batch, dtype=torch.float64, device=dev), where=torch.full((batch, 2), -1, dtype=torch.int32, device=dev))
        if want_rows:
            out["rows"] = torch.empty((batch, sp.nltc + sp.nnltc, ntimes), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_check(self.h, batch, _ptr(x), _ptr(lower), _ptr(upper), ntimes, _ptr(times.contiguous()), stride,
                                     _ptr(out["viol"]), _ptr(out["where"]), _ptr(out.get("rows")), self._stream()))
        return out

    def cost(self, x, times, weights, want_vals: bool = False):
        """The running cost of a batch of trajectories under any quadrature (ntg_batch_cost): x [batch, nC]; times and weights [ntimes]
        or, after set_grids, both [batch, ntimes] (ntg_amd.quadrature builds such pairs).  Returns dict(cost [batch] = sum_i w_i L(t_i)
        [, vals [batch, ntimes] = L(t_i)]).  The initial and final cost are not part of it.  weights may be None with want_vals: the
        result is then dict(vals) alone."""
        import torch
        sp = self.spec
        dev = x.device
        _check_tensor(x, dev)
        if x.dim() != 2 or x.shape[1] != sp.nC:
            raise NtgError(f"x must be [batch, {sp.nC}]")
        batch = x.shape[0]
        if not (times.is_cuda and times.dtype == torch.float64):
            raise NtgError("times must be a float64 tensor on the plan's device")
        if weights is None and not want_vals:
            raise NtgError("nothing asked for: pass weights, want_vals or both")
        if weights is not None and not (weights.is_cuda and weights.dtype == torch.float64 and weights.shape == times.shape):
            raise NtgError("weights must be a float64 tensor on the plan's device, of the shape of times")
        stride = self._times_stride(batch, times)
        ntimes = times.shape[-1]
        out = {}
        if weights is not None:
            out["cost"] = torch.empty(batch, dtype=torch.float64, device=dev)
        if want_vals:
            out["vals"] = torch.empty((batch, ntimes), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_cost(self.h, batch, _ptr(x), ntimes, _ptr(times.contiguous()), _ptr(None if weights is None else weights.contiguous()),
                                    stride, _ptr(out.get("cost")), _ptr(out.get("vals")), self._stream()))
        return out

    def verify(self, x, want_leak: bool = True):
        """Audit the family's analytic derivatives and the plan's active-variable lists at x [batch, nC] (ntg_batch_verify): central
        differences of the six callback slots (icf, ucf, fcf, nlicf, nltcf, nlfcf) at the breakpoints.  Returns dict(err [batch, 6],
        where [batch, 6, 3] = (function, breakpoint, flag entry) [, leak [batch, 6], leak_where [batch, 6, 3]]).  No threshold is applied:
        a wrong derivative shows at the size of its relative error, a correct family at rounding noise."""
        import torch
        sp = self.spec
        dev = x.device
        _check_tensor(x, dev)
        if x.dim() != 2 or x.shape[1] != sp.nC:
            raise NtgError(f"x must be [batch, {sp.nC}]")
        batch = x.shape[0]
        out = dict(err=torch.zeros((batch, 6), dtype=torch.float64, device=dev), where=torch.full((batch, 6, 3), -1, dtype=torch.int32, device=dev))
        if want_leak:
            out["leak"] = torch.zeros((batch, 6), dtype=torch.float64, device=dev)
            out["leak_where"] = torch.full((batch, 6, 3), -1, dtype=torch.int32, device=dev)
        _check(lib().ntg_batch_verify(self.h, batch, _ptr(x), _ptr(out["err"]), _ptr(out["where"]), _ptr(out.get("leak")), _ptr(out.get("leak_where")),
                                      self._stream()))
        return out

    def kkt(self, x, lower, upper, clambda, want_residual: bool = False):
        """First-order optimality residuals of a batch of points (ntg_batch_kkt): x [batch, nC], bounds [batch, nbounds], clambda
        [batch, nC + nclin + ncnln] as solve(want_lambda=True) returns it (its first nC entries are not read).  Returns dict(res
        [batch, 6] = max |r|, max |g|, linear violation, nonlinear violation, signed complementarity, max |lambda|[, r [batch, nC] =
        g - A' lam_A - J' lam_c])."""
        import torch
        sp = self.spec
        dev = x.device
        _check_tensor(x, dev); _check_tensor(lower, dev); _check_tensor(upper, dev); _check_tensor(clambda, dev)
        batch = x.shape[0]
        if x.dim() != 2 or x.shape[1] != sp.nC:
            raise NtgError(f"x must be [batch, {sp.nC}]")
        if lower.shape != (batch, sp.nbounds) or upper.shape != (batch, sp.nbounds):
            raise NtgError(f"bounds must be [{batch}, {sp.nbounds}]")
        if clambda.shape != (batch, sp.nC + sp.nclin + sp.ncnln):
            raise NtgError(f"clambda must be [{batch}, {sp.nC + sp.nclin + sp.ncnln}]")
        out = dict(res=torch.empty((batch, 6), dtype=torch.float64, device=dev))
        if want_residual:
            out["r"] = torch.empty((batch, sp.nC), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_kkt(self.h, batch, _ptr(x), _ptr(lower), _ptr(upper), _ptr(clambda), _ptr(out["res"]), _ptr(out.get("r")),
                                   self._stream()))
        return out

    def refine(self, to: "Plan", x):
        """The same splines on the finer knot grid of plan `to` (ntg_batch_refine): x [batch, nC] -> [batch, to.spec.nC], exact knot
        insertion.  `to` needs the same outputs and orders, every break of this plan among its own, and no more smoothness."""
        import torch
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        _check_tensor(x, torch.device("cuda", self.device))
        if x.dim() != 2 or x.shape[1] != self.spec.nC:
            raise NtgError(f"x must be [batch, {self.spec.nC}]")
        batch = x.shape[0]
        out = torch.empty((batch, to.spec.nC), dtype=torch.float64, device=x.device)
        _check(lib().ntg_batch_refine(self.h, to.h, batch, _ptr(x), _ptr(out), self._stream()))
        return out

    def _cert_inputs(self, x, lower, upper, nsub=0):
        """what envelope, envelope_sos and extrema ask of x [batch, nC], the optional bounds [batch, nbounds] and nsub; -> (spec, device, batch)"""
        sp = self.spec
        dev = x.device
        _check_tensor(x, dev); _check_tensor(lower, dev); _check_tensor(upper, dev)
        if x.dim() != 2 or x.shape[1] != sp.nC:
            raise NtgError(f"x must be [batch, {sp.nC}]")
        batch = x.shape[0]
        if (lower is None) != (upper is None):
            raise NtgError("pass both bounds or neither")
        if lower is not None and (lower.shape != (batch, sp.nbounds) or upper.shape != (batch, sp.nbounds)):
            raise NtgError(f"bounds must be [{batch}, {sp.nbounds}]")
        if not 0 <= int(nsub) <= ENVELOPE_MAX_NSUB:
            raise NtgError(f"nsub must lie in 0 .. {ENVELOPE_MAX_NSUB} (NTG_ENVELOPE_MAX_NSUB)")
        return sp, dev, batch

    def envelope(self, x, nsub: int = 0, lower=None, upper=None, want_entries: bool = True, want_rows: bool = False):
        """Bounds of a batch of trajectories that hold at EVERY time (ntg_batch_envelope): x [batch, nC]; every knot interval is cut into
        2^nsub pieces, npc = max(kninterv) << nsub (envelope_pieces gives their ends).  Returns a dict: lo, hi [batch, nz, npc] (the flag
        entries, want_entries), row_lo, row_hi [batch, nltc, npc] (the linear trajectory rows, want_rows), and with bounds [batch, nbounds]
        viol [batch] and where [batch, 2] = (row, piece) of the largest certified violation or (-1, -1).  Pieces past an output's own are
        the empty set (lo = +inf, hi = -inf).  viol == 0 certifies every linear trajectory row over the whole horizon."""
        import torch
        sp, dev, batch = self._cert_inputs(x, lower, upper, nsub)
        if (want_rows or lower is not None) and sp.nltc == 0:   # (empty row tensors would reach the library as null pointers)
            raise NtgError("the plan has no linear trajectory rows (nltc == 0): there is no row envelope and no violation to ask for")
        npc = max(sp.kninterv) << int(nsub)
        out = {}
        if want_entries:
            out["lo"] = torch.empty((batch, sp.nz, npc), dtype=torch.float64, device=dev); out["hi"] = torch.empty_like(out["lo"])
        if want_rows:
            out["row_lo"] = torch.empty((batch, sp.nltc, npc), dtype=torch.float64, device=dev); out["row_hi"] = torch.empty_like(out["row_lo"])
        if lower is not None:
            out["viol"] = torch.zeros(batch, dtype=torch.float64, device=dev); out["where"] = torch.full((batch, 2), -1, dtype=torch.int32, device=dev)
        _check(lib().ntg_batch_envelope(self.h, batch, _ptr(x), int(nsub), _ptr(lower), _ptr(upper), _ptr(out.get("lo")), _ptr(out.get("hi")),
                                        _ptr(out.get("row_lo")), _ptr(out.get("row_hi")), _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def sos_rows(self) -> np.ndarray:
        """[nnltc] int32: 1 where envelope_sos certifies the nonlinear trajectory row on this plan, 0 where it makes no statement (the
        family does not declare the row a sum of squares, or the row names outputs of different basis classes).  See ntg_plan_sos_rows."""
        flags = np.zeros(self.spec.nnltc, dtype=np.int32)
        _check(lib().ntg_plan_sos_rows(self.h, flags.ctypes.data_as(ip)))
        return flags

    def envelope_sos(self, x, nsub: int = 0, lower=None, upper=None):
        """Bounds of the sum-of-squares trajectory rows (obstacle clearance, thrust^2, speed^2) that hold at EVERY time
        (ntg_batch_envelope_sos): x [batch, nC]; pieces as in envelope.  Returns a dict: q_lo, q_hi [batch, nnltc, npc] and, with bounds
        [batch, nbounds], viol [batch] and where [batch, 2] = (row, piece) of the largest certified violation or (-1, -1).  A row
        sos_rows() flags 0 comes back as (-inf, +inf) on its live pieces, and viol / where are then refused.  viol == 0 certifies every
        nonlinear trajectory row over the whole horizon."""
        import torch
        sp, dev, batch = self._cert_inputs(x, lower, upper, nsub)
        npc = max(sp.kninterv) << int(nsub)
        # (a plan without such rows gets one row of storage: the library refuses it before it writes, an empty tensor would arrive as a null pointer)
        out = {"q_lo": torch.empty((batch, max(sp.nnltc, 1), npc), dtype=torch.float64, device=dev)}
        out["q_hi"] = torch.empty_like(out["q_lo"])
        if lower is not None:
            out["viol"] = torch.zeros(batch, dtype=torch.float64, device=dev); out["where"] = torch.full((batch, 2), -1, dtype=torch.int32, device=dev)
        _check(lib().ntg_batch_envelope_sos(self.h, batch, _ptr(x), int(nsub), _ptr(lower), _ptr(upper), _ptr(out["q_lo"]), _ptr(out["q_hi"]),
                                            _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def extrema_rows(self) -> np.ndarray:
        """[nltc + nnltc] int32: 1 where extrema certifies the trajectory row on this plan (a linear row whose outputs share a basis class,
        a nonlinear row sos_rows() flags), 0 where it makes no statement.  See ntg_plan_extrema_rows."""
        flags = np.zeros(self.spec.nltc + self.spec.nnltc, dtype=np.int32)
        _check(lib().ntg_plan_extrema_rows(self.h, flags.ctypes.data_as(ip)))
        return flags

    def extrema(self, x, tol, max_depth: int = 30, sides: int = 3, lower=None, upper=None):
        """The minimum and maximum of every certifiable trajectory row over the whole horizon, each enclosed to tol, by bisection
        (ntg_batch_extrema): x [batch, nC]; rows are the nltc linear trajectory rows, then the nnltc nonlinear ones.  Returns a dict: ext
        [batch, nrow, 4] = (min_lo, min_hi, max_lo, max_hi), when [batch, nrow, 2] = (t_min, t_max), the times where min_hi and max_lo are
        attained, status [batch, nrow] (EXTREMA_OK / _DEPTH / _FULL / _NAN / _NONE), npieces [batch, nrow] and, with bounds [batch, nbounds],
        viol [batch, 2] = (attained, certified) and where [batch, 2], the row of each or -1.  sides: 1 the minimum, 2 the maximum, 3 both.
        viol[:, 1] == 0 certifies every trajectory row over the whole horizon; a row extrema_rows() flags 0 comes back as
        (-inf, +inf, -inf, +inf), and viol / where are then refused."""
        sp, dev, batch = self._cert_inputs(x, lower, upper)
        out = _bisect_out(batch, sp.nltc + sp.nnltc, dev, lower is not None)
        _check(lib().ntg_batch_extrema(self.h, batch, _ptr(x), float(tol), int(max_depth), int(sides), _ptr(lower), _ptr(upper), _ptr(out["ext"]), _ptr(out["when"]),
                                       _ptr(out["status"]), _ptr(out["npieces"]), _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def separation(self, x, pairs, bodies, deriv: int = 0, tol: float = 0.0, max_depth: int = 30, sep=None):
        """The closest approach of pairs of planned bodies over the whole horizon, enclosed to tol, by bisection (ntg_batch_separation):
        x [batch, nC]; bodies [nbody, ndim] (host, integers) names the outputs that are the coordinates of every body, e.g. [[0, 1], [2, 3],
        [4, 5]] for three cars; pairs [npairs, 4] int32 on the device = (a, b, ga, gb), body ga of problem a against body gb of problem b
        (a == b: two cars of one problem).  deriv = 0: the distance of positions, 1: the relative speed.  sep [npairs] (device) or None: the
        required distances.  Returns a dict: min [npairs, 2] = (min_lo, min_hi) of the SQUARED distance, when [npairs] the time where min_hi
        is attained, status [npairs] (EXTREMA_OK / _DEPTH / _FULL / _NAN, or SEP_BADPAIR for indices out of range), npieces [npairs] and,
        with sep, viol [npairs, 2] = (attained, certified) = max(sep^2 - min_hi, 0), max(sep^2 - min_lo, 0): viol[:, 1] == 0 certifies the
        separation over the whole horizon.  With sep, a piece that cannot come closer than required retires at once."""
        import torch
        sp, dev, batch = self._cert_inputs(x, None, None)
        _check_tensor(pairs, dev, torch.int32); _check_tensor(sep, dev)
        body = np.ascontiguousarray(np.asarray(bodies, dtype=np.int32))
        if body.ndim != 2 or body.size == 0:
            raise NtgError("bodies must be [nbody, ndim] output indices")
        if pairs.dim() != 2 or pairs.shape[1] != 4:
            raise NtgError("pairs must be an int32 tensor [npairs, 4] = (a, b, ga, gb)")
        npairs = pairs.shape[0]
        if sep is not None and sep.shape != (npairs,):
            raise NtgError(f"sep must be [{npairs}]")
        out = {"min": torch.empty((npairs, 2), dtype=torch.float64, device=dev), "when": torch.empty(npairs, dtype=torch.float64, device=dev),
               "status": torch.empty(npairs, dtype=torch.int32, device=dev), "npieces": torch.empty(npairs, dtype=torch.int32, device=dev)}
        if sep is not None:
            out["viol"] = torch.empty((npairs, 2), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_separation(self.h, batch, _ptr(x), body.shape[0], body.shape[1], body.ctypes.data_as(ip), int(deriv), npairs, _ptr(pairs), _ptr(sep),
                                          float(tol), int(max_depth), _ptr(out["min"]), _ptr(out["when"]), _ptr(out["status"]), _ptr(out["npieces"]), _ptr(out.get("viol")),
                                          self._stream()))
        return out

    def forms(self, x, forms, tol, max_depth: int = 30, sides: int = 3, fprm=None, lower=None, upper=None):
        """The minimum and maximum over the whole horizon of quadratic forms of the flat flag declared here, each enclosed to tol, by bisection
        (ntg_batch_forms): x [batch, nC]; forms is a list of up to FORM_MAXFORMS forms, each a list of up to FORM_MAXTERMS terms (u, v, pu, pv,
        w, su, sv) as the constructors of ntg_amd.forms return them: w (z[u] - a)(z[v] - b), or w (z[u] - a) for v == -1, with a = su +
        fprm[b, pu] and b = sv + fprm[b, pv].  fprm [batch, nfp] (device) are the call's own per-problem parameters.  No family callback runs,
        so every plan is served, loaded modules and per-problem grids included.  Returns a dict like extrema's: ext [batch, nform, 4] =
        (min_lo, min_hi, max_lo, max_hi), when [batch, nform, 2], status and npieces [batch, nform] and, with the bounds lower / upper
        [batch, nform] of the forms, viol [batch, 2] = (attained, certified) and where [batch, 2], the form of each or -1.
        viol[:, 1] == 0 certifies every declared form over the whole horizon."""
        sp, dev, batch = self._cert_inputs(x, None, None)
        forms = list(forms)
        nform = len(forms)
        nterms, terms, nfp = _declare_forms(forms, fprm, lower, upper, dev, batch, nform, "forms")
        out = _bisect_out(batch, nform, dev, lower is not None)
        _check(lib().ntg_batch_forms(self.h, batch, _ptr(x), nform, nterms, terms, nfp, _ptr(fprm), float(tol), int(max_depth),
                                     int(sides), _ptr(lower), _ptr(upper), _ptr(out["ext"]), _ptr(out["when"]), _ptr(out["status"]), _ptr(out["npieces"]),
                                     _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def ratios(self, x, forms, ratios, tol, max_depth: int = 30, sides: int = 3, fprm=None, lower=None, upper=None):
        """The minimum and maximum over the whole horizon of ratios of products of quadratic forms of the flat flag, each enclosed to tol, by
        bisection of pairs of polygons (ntg_batch_ratios): forms as for Plan.forms; ratios is a list of up to RATIO_MAXRATIOS pairs (num, den)
        of lists of up to RATIO_MAXFACTORS form indices, as ntg_amd.forms.ratio returns them: the product of the forms num over the product of
        the forms den (an empty list is 1, a repeated index a power).  Returns the dict of Plan.forms with the ratio in the place of the form;
        status RATIO_POLE: the denominator was <= 0 at a time the bisection visited, no statement.  lower / upper [batch, nratio]."""
        sp, dev, batch = self._cert_inputs(x, None, None)
        forms, ratios = list(forms), [(list(n), list(d)) for n, d in ratios]
        nform, nratio = len(forms), len(ratios)
        nterms, terms, nfp = _declare_forms(forms, fprm, lower, upper, dev, batch, nratio, "ratios", ratios)
        pad = lambda v: (C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))
        rat = (Ratio * max(nratio, 1))(*[Ratio(len(n), len(d), pad(n), pad(d)) for n, d in ratios])
        out = _bisect_out(batch, nratio, dev, lower is not None)
        _check(lib().ntg_batch_ratios(self.h, batch, _ptr(x), nform, nterms, terms, nfp, _ptr(fprm), nratio, rat, float(tol),
                                      int(max_depth), int(sides), _ptr(lower), _ptr(upper), _ptr(out["ext"]), _ptr(out["when"]), _ptr(out["status"]), _ptr(out["npieces"]),
                                      _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def trig(self, x, forms, tol, max_depth: int = 30, sides: int = 3, fprm=None, lower=None, upper=None):
        """The minimum and maximum over the whole horizon of sums of sines and cosines of the flat flag declared here, each enclosed to tol, by
        bisection (ntg_batch_trig): forms is a list of up to TRIG_MAXFORMS forms, each a list of up to TRIG_MAXTERMS ntg_amd.trig.Term
        (kind, ent, coef, phase, pp, w): w g(theta), theta = sum_i coef[i] z[ent[i]] + phase + fprm[b, pp], g = sin, cos or the identity.  The
        constructors of ntg_amd.trig build them (tip_height, tip_x, wall, heading).  No family callback runs: the manipulator's rows, which
        Plan.extrema refuses, are certified this way.  Returns the dict of Plan.forms; lower / upper [batch, nform]."""
        sp, dev, batch = self._cert_inputs(x, None, None)
        forms = [list(f) for f in forms]
        nform = len(forms)
        _declare_forms([], fprm, lower, upper, dev, batch, nform, "forms")
        for f, form in enumerate(forms):
            for t, q in enumerate(form):
                if not 1 <= len(q.ent) <= TRIG_MAXENT or len(q.ent) != len(q.coef):
                    raise NtgError(f"form {f}, term {t}: 1 .. {TRIG_MAXENT} entries with one coef each")
        pad = lambda v, ty: (ty * 4)(*(list(v) + [0] * (4 - len(v))))
        flat = [TrigTerm(int(q.kind), len(q.ent), int(q.pp), 0, pad([int(e) for e in q.ent], C.c_int), pad([float(c) for c in q.coef], C.c_double), float(q.phase), float(q.w))
                for form in forms for q in form]
        nterms = (C.c_int * max(nform, 1))(*[len(f) for f in forms])
        terms = (TrigTerm * max(len(flat), 1))(*flat)
        out = _bisect_out(batch, nform, dev, lower is not None)
        _check(lib().ntg_batch_trig(self.h, batch, _ptr(x), nform, nterms, terms, 0 if fprm is None else int(fprm.shape[1]), _ptr(fprm), float(tol), int(max_depth),
                                    int(sides), _ptr(lower), _ptr(upper), _ptr(out["ext"]), _ptr(out["when"]), _ptr(out["status"]), _ptr(out["npieces"]),
                                    _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def minmax(self, x, forms, groups, tol, max_depth: int = 30, sides: int = 3, fprm=None, lower=None, upper=None):
        """The minimum and maximum over the whole horizon of min / max expressions over quadratic forms of the flat flag, each enclosed to tol,
        by bisection of pieces that carry the polygons of all members (ntg_batch_minmax): forms as for Plan.forms (up to MINMAX_MAXFORMS, 40
        terms together); groups is a list of up to MINMAX_MAXGROUPS triples (outer, inner, clauses), clauses a list of lists of members
        (form, c, pc): h = OUTER over the clauses of INNER over the clause's members of q_form(z) + c + fprm[b, pc].  The constructors of
        ntg_amd.minmax build both (polygon, box, corridor, discs, merge).  Returns the dict of Plan.forms with the group in the place of the
        form, plus which [batch, ngroup, 2]: the member, by its index in the group's concatenated list, that decides h at t_min and at t_max.
        lower / upper [batch, ngroup]; viol[:, 1] == 0 certifies every group over the whole horizon."""
        import torch
        sp, dev, batch = self._cert_inputs(x, None, None)
        forms = list(forms)
        groups = [(int(o), int(i), [[(int(f), float(c), int(pc)) for f, c, pc in cl] for cl in cls]) for o, i, cls in groups]
        nform, ngroup = len(forms), len(groups)
        nterms, terms, nfp = _declare_forms(forms, fprm, lower, upper, dev, batch, ngroup, "groups")
        for g, (o, i, cls) in enumerate(groups):
            if len(cls) > MINMAX_MAXCLAUSES:
                raise NtgError(f"group {g}: nclause = {len(cls)} must lie in 1 .. {MINMAX_MAXCLAUSES}")
        pad = lambda v: (C.c_int * 8)(*(list(v) + [0] * (8 - len(v))))
        grp = (MinmaxGroup * max(ngroup, 1))(*[MinmaxGroup(o, i, len(cls), 0, pad([len(cl) for cl in cls])) for o, i, cls in groups])
        flat = [MinmaxMember(f, pc, c) for _, _, cls in groups for cl in cls for f, c, pc in cl]
        mem = (MinmaxMember * max(len(flat), 1))(*flat)
        out = _bisect_out(batch, ngroup, dev, lower is not None)
        out["which"] = torch.empty((batch, max(ngroup, 1), 2), dtype=torch.int32, device=dev)
        _check(lib().ntg_batch_minmax(self.h, batch, _ptr(x), nform, nterms, terms, nfp, _ptr(fprm), ngroup, grp, mem, float(tol), int(max_depth), int(sides),
                                      _ptr(lower), _ptr(upper), _ptr(out["ext"]), _ptr(out["when"]), _ptr(out["which"]), _ptr(out["status"]), _ptr(out["npieces"]),
                                      _ptr(out.get("viol")), _ptr(out.get("where")), self._stream()))
        return out

    def set_grids(self, knots, bps, with_precond: bool = True):
        """Per-problem grids: knots [batch, ninterv+1], bps [batch, nbps] (device, float64).  See ntg_plan_set_grids."""
        _check_tensor(knots, knots.device); _check_tensor(bps, bps.device)
        if knots.shape[0] != bps.shape[0] or knots.shape[1] != self.spec.kninterv[0] + 1 or bps.shape[1] != self.spec.nbps:
            raise NtgError("knots must be [batch, ninterv+1] and bps [batch, nbps]")
        _check(lib().ntg_plan_set_grids(self.h, knots.shape[0], _ptr(knots), _ptr(bps), int(with_precond), self._stream()))
        self.grid_batch = int(knots.shape[0])

    def clear_grids(self):
        lib().ntg_plan_clear_grids(self.h)
        self.grid_batch = 0

    @property
    def param_count(self) -> int:
        """doubles of per-problem parameters the plan's family reads (0: it takes none).  See ntg_plan_param_count."""
        n = C.c_int()
        _check(lib().ntg_plan_param_count(self.h, C.byref(n)))
        return n.value

    def set_params(self, params):
        """Per-problem family parameters: params [batch, param_count] (device, float64), copied into the plan.  Eval, solve and mpc_run
        then take exactly `batch` problems.  See ntg_plan_set_params."""
        import torch
        _check_tensor(params, torch.device("cuda", self.device))
        if params.dim() != 2 or params.shape[1] != self.param_count:
            raise NtgError(f"params must be [batch, {self.param_count}]")
        _check(lib().ntg_plan_set_params(self.h, params.shape[0], params.shape[1], _ptr(params), self._stream()))
        self.param_batch = int(params.shape[0])

    def clear_params(self):
        lib().ntg_plan_clear_params(self.h)
        self.param_batch = 0

    def kincar_reverse(self, z, wheelbase: float = 3.0, reverse_gear: bool = False):
        """Flat flag -> (x, y, theta, v, delta) per car: z [batch, ntimes, nz] (from interp) -> [batch, ntimes, ncars, 5]."""
        import torch
        _check_tensor(z, z.device)
        out = torch.empty((z.shape[0], z.shape[1], self.spec.nout // 2, 5), dtype=torch.float64, device=z.device)
        _check(lib().ntg_batch_kincar_reverse(self.h, z.shape[0], z.shape[1], _ptr(z), C.c_double(wheelbase), int(reverse_gear), _ptr(out), self._stream()))
        return out

    def mpc_shift(self, x, lower, upper, shift_bp: int, shift_knots: int):
        """Receding-horizon step in place: re-pin initial bounds to the solution's flag at breakpoint
        shift_bp, shift the coefficients by shift_knots knot intervals."""
        _check(lib().ntg_batch_mpc_shift(self.h, x.shape[0], shift_bp, shift_knots, _ptr(x), _ptr(lower), _ptr(upper), self._stream()))

    def mpc_shift_multipliers(self, batch: int, shift_bp: int, opts: SolveOpts, work):
        """The multipliers' share of the receding-horizon step: estimates in `work` move shift_bp breakpoints towards the start of the horizon."""
        _check(lib().ntg_batch_mpc_shift_multipliers(self.h, batch, shift_bp, C.byref(opts), _ptr(work), work.numel() * work.element_size(), self._stream()))

    def mpc_run(self, x, lower, upper, nsteps: int, shift_bp: int, shift_knots: int, opts: Optional[SolveOpts] = None, work=None):
        """nsteps x (solve, shift) inside the library (hipGraph replay).  Returns (inform of the last step, #not converged)."""
        import torch
        o = opts if opts is not None else default_opts()
        batch = x.shape[0]
        need = self.workspace_bytes(batch, o)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=x.device)
        inform = torch.empty(batch, dtype=torch.int32, device=x.device)
        bad = torch.zeros(1, dtype=torch.int32, device=x.device)
        torch.cuda.current_stream().synchronize()
        _check(lib().ntg_batch_mpc_run(self.h, batch, nsteps, shift_bp, shift_knots, _ptr(x), _ptr(lower), _ptr(upper), C.byref(o),
                                       _ptr(inform), _ptr(bad), _ptr(work), work.numel() * work.element_size(), self._stream()))
        return inform, bad

    def solve_kernel(self, batch: int, opts: Optional[SolveOpts] = None) -> str:
        """name of the kernel solve() launches for this batch and these options"""
        return lib().ntg_batch_solve_kernel(self.h, batch, C.byref(opts) if opts is not None else None).decode()

    def workspace_bytes(self, batch: int, opts: Optional[SolveOpts] = None) -> int:
        return int(lib().ntg_batch_workspace_bytes(self.h, batch, C.byref(opts) if opts is not None else None))

    def solve(self, lower, upper, x, opts: Optional[SolveOpts] = None, work=None, out=None, want_lambda: bool = False):
        """In place on x.  Returns dict(objective, inform, iters, nfev[, clambda])."""
        import torch
        sp = self.spec
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        assert lower.is_contiguous() and upper.is_contiguous()
        batch = x.shape[0]
        dev = x.device
        o = opts if opts is not None else default_opts()
        need = self.workspace_bytes(batch, o)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=dev)
        assert work.numel() * work.element_size() >= need
        _check_tensor(lower, dev); _check_tensor(upper, dev)
        if lower.shape != (batch, sp.nbounds) or upper.shape != (batch, sp.nbounds):
            raise NtgError(f"bounds must be [{batch}, {sp.nbounds}]")
        if out is not None:
            _check_tensor(out["objective"], dev)
            for k in ("inform", "iters", "nfev"):
                _check_tensor(out[k], dev, torch.int32)
            _check_tensor(out.get("clambda"), dev)
        if out is None:
            out = dict(objective=torch.empty(batch, dtype=torch.float64, device=dev),
                       inform=torch.empty(batch, dtype=torch.int32, device=dev),
                       iters=torch.empty(batch, dtype=torch.int32, device=dev),
                       nfev=torch.empty(batch, dtype=torch.int32, device=dev))
            if want_lambda:
                out["clambda"] = torch.empty((batch, sp.nC + sp.nclin + sp.ncnln), dtype=torch.float64, device=dev)
        _check(lib().ntg_batch_solve(self.h, batch, _ptr(lower), _ptr(upper), _ptr(x), C.byref(o),
                                     _ptr(out["objective"]), _ptr(out["inform"]), _ptr(out["iters"]), _ptr(out["nfev"]),
                                     _ptr(out.get("clambda")), _ptr(work), work.numel() * work.element_size(), self._stream()))
        return out


ENVELOPE_MAX_NSUB = 6   # NTG_ENVELOPE_MAX_NSUB
EXTREMA_MAX_DEPTH, EXTREMA_CAP = 30, 64   # NTG_EXTREMA_MAX_DEPTH, NTG_EXTREMA_CAP
EXTREMA_OK, EXTREMA_DEPTH, EXTREMA_FULL, EXTREMA_NAN, EXTREMA_NONE = 0, 1, 2, 3, -1   # NTG_EXTREMA_* status codes
SEP_MAXDIM, SEP_BADPAIR = 4, -2   # NTG_SEP_MAXDIM, NTG_SEP_BADPAIR
FORM_MAXFORMS, FORM_MAXTERMS = 8, 8   # NTG_FORM_MAXFORMS, NTG_FORM_MAXTERMS
RATIO_MAXRATIOS, RATIO_MAXFACTORS, RATIO_MAXDEG, RATIO_POLE = 4, 4, 24, 4   # NTG_RATIO_MAXRATIOS, _MAXFACTORS, _MAXDEG; status NTG_RATIO_POLE


def envelope_pieces(spec_or_knots, o: int = 0, nsub: int = 0) -> np.ndarray:
    """The ends [npc + 1] of the pieces Plan.envelope reports for output o: piece q of that output covers [ends[q], ends[q + 1]].  Takes a
    Spec (npc = max(kninterv) << nsub; the entries past the output's own pieces are NaN) or one break sequence [l + 1] (npc = l << nsub,
    e.g. a problem's own knots after set_grids)."""
    if hasattr(spec_or_knots, "knots"):
        kn = np.asarray(spec_or_knots.knots[o], dtype=np.float64); npc = max(spec_or_knots.kninterv) << nsub
    else:
        kn = np.asarray(spec_or_knots, dtype=np.float64); npc = (len(kn) - 1) << nsub
    n = 1 << nsub
    a, h = kn[:-1], np.diff(kn)
    ends = np.full(npc + 1, np.nan)
    own = (a[:, None] + h[:, None] * (np.arange(n)[None, :] / n)).reshape(-1)
    ends[:own.size] = own
    ends[own.size] = kn[-1]
    return ends


def load_family(path: str) -> int:
    """Load a family module (ntg_amd.family.build_module) and return its id for Spec.family.  The same file loaded again returns
    the same id.  Needs no GPU."""
    fam = C.c_int()
    _check(lib().ntg_family_load(os.fsencode(path), C.byref(fam)))
    return fam.value


def family_info(family: int) -> dict:
    """What a loaded module declares: name, maxderiv, the most nonlinear rows of each kind, the outputs a plan must have (0: any)."""
    name = C.create_string_buffer(256)
    v = [C.c_int() for _ in range(5)]
    _check(lib().ntg_family_info(family, name, len(name), *[C.byref(x) for x in v]))
    return dict(name=name.value.decode(), maxderiv=v[0].value, nnlic=v[1].value, nnltc=v[2].value, nnlfc=v[3].value, nout=v[4].value)


def basis_batch(knots, bps, order: int, mult: int, maxderiv: int):
    """bsplvd at every collocation point of many grids: knots [G, l+1], bps [G, P] (torch, device)."""
    import torch
    G, l1 = knots.shape
    P = bps.shape[1]
    blk = torch.empty((G, P, order, maxderiv), dtype=torch.float64, device=knots.device)
    off = torch.empty((G, P), dtype=torch.int32, device=knots.device)
    _check(lib().ntg_basis_batch(G, l1 - 1, order, mult, maxderiv, P, _ptr(knots), _ptr(bps), _ptr(blk), _ptr(off),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return blk, off
