"""-m gpu: ntg_batch_kkt, the first-order optimality residuals of a batch on the device.

The yardstick of every arithmetic test is numpy on outputs of calls that existed before it: Plan.eval(x, 2, want_dense_jac=True) for g, c
and the dense Jacobian, Plan.tables() / Plan.grid_tables(b) for A, Plan.bounds for (bl, bu), and the definitions of include/ntg_amd.h
restated below (kkt_numpy).  Inputs are random points and random multipliers (half of them exact zeros, mixed signs), bounds tampered per
slot: one-sided, absent, lower == upper, windows that hold every row of the slot and windows that miss even the row they were drawn from.

Tolerances (from the summation lengths, not measured): an entry of r sums at most a few hundred products, n x 2.2e-16 relative to the sum
of their magnitudes, so 1e-12 x (|g| + |A|'|lam_A| + |J|'|lam_c|) leaves a tenfold margin; res[0] to the largest of these bounds; a . x
to 1e-12 x (|A||x|); res[1], res[3], res[5] are maxima of absolute values or single subtractions of identical inputs: bit-equal."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from ntg_amd import api, configs as cf
from gpu_common import dev
from test_gpu_grids import grids_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 1e20   # NTG_INF_BOUND


def kkt_numpy(g, c, J, A, x, bl, bu, lam):
    """the definitions of ntg_batch_kkt for one problem: (r, res[6], per-entry scale of r, largest (|A||x|)_r)"""
    nC, nclin = x.size, A.shape[0]
    lA, lc = lam[nC:nC + nclin], lam[nC + nclin:]
    r = g - A.T @ lA - (J.T @ lc if lc.size else 0.0)
    scale = np.abs(g) + np.abs(A).T @ np.abs(lA) + (np.abs(J).T @ np.abs(lc) if lc.size else 0.0)
    v = np.concatenate([A @ x, c]); lo, up = bl[nC:], bu[nC:]; lr = lam[nC:]
    hl, hu = np.abs(lo) < INF, np.abs(up) < INF
    with np.errstate(over="ignore", invalid="ignore"):
        viol = np.maximum(np.maximum(np.where(hl, lo - v, 0.0), np.where(hu, v - up, 0.0)), 0.0)
        slo = np.where(hl, np.clip(v - lo, 0.0, 1.0), 1.0); sup = np.where(hu, np.clip(up - v, 0.0, 1.0), 1.0)
    comp = np.maximum(lr, 0.0) * slo + np.maximum(-lr, 0.0) * sup
    res = np.array([np.abs(r).max(), np.abs(g).max(), viol[:nclin].max(initial=0.0), viol[nclin:].max(initial=0.0),
                    comp.max(initial=0.0), np.abs(lr).max(initial=0.0)])
    return r, res, scale, (np.abs(A) @ np.abs(x)).max(initial=0.0)


def slot_of_row(p, spec):
    """bound slot of every linear and nonlinear row, read off Plan.bounds' own expansion"""
    idx = np.arange(spec.nbounds, dtype=np.float64)[None]
    return p.bounds(dev(idx), dev(idx))[0][0, spec.nC:].cpu().numpy().astype(int)


def make_inputs(p, spec, nb, seed, A_of=None):
    """random x, multipliers and tampered bounds; everything the numpy side needs, evaluated once"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nb, spec.nC)) * 0.5 + 1.0
    x[nb // 2] *= 3.0                                           # one problem pushed far out: its rows are violated by a lot
    ntot = spec.nC + spec.nclin + spec.ncnln
    lam = rng.normal(size=(nb, ntot)) * (rng.random((nb, ntot)) < 0.5)
    lam[:, :spec.nC] = rng.normal(size=(nb, spec.nC)) * 1e3     # never read
    ev = p.eval(dev(x), 2, want_dense_jac=True)
    g = ev["g"].cpu().numpy()
    c = ev["c"].cpu().numpy() if spec.ncnln else np.zeros((nb, 0))
    J = ev["cJac"].cpu().numpy() if spec.ncnln else np.zeros((nb, 0, spec.nC))
    As = [A_of(b) if A_of else None for b in range(nb)]
    if A_of is None:
        As = [p.tables()["A"]] * nb
    slot = slot_of_row(p, spec)
    lo = np.empty((nb, spec.nbounds)); up = np.empty_like(lo)
    for b in range(nb):
        v = np.concatenate([As[b] @ x[b], c[b]])
        for s in range(spec.nbounds):
            vs = v[slot == s]; vmin, vmax = vs.min(), vs.max(); mid = vs[rng.integers(vs.size)]
            kind = rng.integers(8)   # (mid is one of the slot's own row values: kinds 6 and 7 violate a slot of a single row too)
            if kind == 0: lo[b, s], up[b, s] = -INF, mid + 0.25
            elif kind == 1: lo[b, s], up[b, s] = mid - 0.25, INF
            elif kind == 2: lo[b, s] = up[b, s] = mid
            elif kind == 3: lo[b, s], up[b, s] = -INF, INF
            elif kind == 4: lo[b, s], up[b, s] = vmin - 0.5, vmax + 0.5
            elif kind == 5: lo[b, s], up[b, s] = mid - 0.3, mid + 0.6
            elif kind == 6: lo[b, s], up[b, s] = mid + 0.2, mid + 0.9      # the row sits 0.2 under its lower bound
            else: lo[b, s], up[b, s] = -INF, mid - 0.4                     # the row sits 0.4 over its upper bound
    bl, bu = p.bounds(dev(lo), dev(up))
    return dict(x=x, lam=lam, lo=lo, up=up, g=g, c=c, J=J, A=As, bl=bl.cpu().numpy(), bu=bu.cpu().numpy())


def compare(spec, d, out):
    res = out["res"].cpu().numpy(); r = out["r"].cpu().numpy()
    kinds = set()
    for b in range(d["x"].shape[0]):
        rn, resn, scale, ax = kkt_numpy(d["g"][b], d["c"][b], d["J"][b], d["A"][b], d["x"][b], d["bl"][b], d["bu"][b], d["lam"][b])
        err = np.abs(r[b] - rn)
        print(f"problem {b}: |r - r_np| / scale max {np.max(err / np.maximum(scale, 1e-300)):.2e}  res {res[b]}  numpy {resn}")
        assert (err <= 1e-12 * scale).all(), (b, np.max(err / np.maximum(scale, 1e-300)))
        assert abs(res[b, 0] - resn[0]) <= 1e-12 * scale.max(), (b, res[b, 0], resn[0])
        for i in (1, 3, 5):
            assert res[b, i] == resn[i], (b, i, res[b, i], resn[i])
        assert abs(res[b, 2] - resn[2]) <= 1e-12 * ax, (b, res[b, 2], resn[2])
        assert abs(res[b, 4] - resn[4]) <= 1e-12 * resn[5] * max(1.0, ax), (b, res[b, 4], resn[4])
        kinds |= {i for i in range(6) if resn[i] > 0}
    return kinds


def run(p, d, want_residual=True):
    return p.kkt(dev(d["x"]), dev(d["lo"]), dev(d["up"]), dev(d["lam"]), want_residual=want_residual)


@pytest.fixture(scope="module")
def unicycle():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))


def _linineq_spec():
    s = cf.config_B()
    flags = [0] * 12; flags[6 + 3] = 1; flags[6 + 5] = 1     # the plan of tests/test_gpu_linineq.py
    s.lin_ineq = flags
    return s


CASES = {"T": (cf.config_T, 5), "D8": (lambda: cf.config_D(ninterv=8), 6), "E8": (lambda: cf.config_E(ninterv=8), 4), "K0": (cf.config_K0, 5),
         "linineq": (_linineq_spec, 5), "OF3": (lambda: cf.config_OF(3), 5), "U": (None, 5)}
_cache = {}


def case(name, unicycle=None):
    """(spec, plan, inputs) of a case, built once for the module"""
    if name not in _cache:
        mk, nb = CASES[name]
        spec = cf.config_U(unicycle) if name == "U" else mk()
        p = api.Plan(spec, 0)
        if name == "OF3":
            p.set_params(dev(cf.obstacle_field_problems(nb, 3, seed=99)[0]))
        _cache[name] = (spec, p, make_inputs(p, spec, nb, seed=20 + len(_cache)))
    return _cache[name]


# -- 1. arithmetic against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_arithmetic_against_numpy(name, unicycle):
    spec, p, d = case(name, unicycle)
    out = run(p, d)
    torch.cuda.synchronize()
    kinds = compare(spec, d, out)
    # every figure carries weight in the inputs (the nonlinear violation only where there are nonlinear rows)
    assert kinds >= ({0, 1, 2, 4, 5} | ({3} if spec.ncnln else set())), kinds
    if not spec.ncnln:
        assert (out["res"][:, 3] == 0).all()
    only = run(p, d, want_residual=False)
    assert torch.equal(only["res"], out["res"]) and "r" not in only


# -- 2. per-problem grids ----------------------------------------------------------------------------------------------------------------
def test_per_problem_grids():
    spec = cf.config_O(ninterv=8)
    nb = 8
    knots, bps = grids_for(spec, nb, warp=0.2)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    d = make_inputs(p, spec, nb, seed=7, A_of=lambda b: p.grid_tables(b)["A"])
    assert np.abs(d["A"][0] - d["A"][1]).max() > 1e-3     # the rows do differ from problem to problem
    out = run(p, d)
    compare(spec, d, out)
    with pytest.raises(api.NtgError, match="-2"):          # the grids are for exactly this batch
        p.kkt(dev(d["x"][:3]), dev(d["lo"][:3]), dev(d["up"][:3]), dev(d["lam"][:3]))


# -- 3. chunks ---------------------------------------------------------------------------------------------------------------------------
def _debug_kkt(p, d, cap):
    L = api.lib()
    L.ntg_debug_batch_kkt.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_longlong]
    nb, nC = d["x"].shape
    t = [dev(d[k]) for k in ("x", "lo", "up", "lam")]
    res = torch.full((nb, 6), -1.0, dtype=torch.float64, device="cuda:0"); r = torch.full((nb, nC), -1.0, dtype=torch.float64, device="cuda:0")
    rc = L.ntg_debug_batch_kkt(p.h, nb, *[x.data_ptr() for x in t], res.data_ptr(), r.data_ptr(), None, cap)
    assert rc == 0, L.ntg_last_error()
    torch.cuda.synchronize()
    return res, r


def test_chunks_are_bit_identical():
    spec = cf.config_E(ninterv=8)
    p = api.Plan(spec, 0)
    d = make_inputs(p, spec, 8, seed=3)
    per = 8 * (1 + spec.nC + spec.ncnln * (1 + spec.sumk) + 2 * (spec.nC + spec.nclin + spec.ncnln))   # scratch bytes of one problem
    one = _debug_kkt(p, d, 1 << 40)
    for cap in (per + per // 2, 3 * per + per // 2, 1):     # chunks of 1, of 3 + 3 + 2, and a cap below one problem (still one per chunk)
        got = _debug_kkt(p, d, cap)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), cap
    out = run(p, d)
    assert torch.equal(out["res"], one[0]) and torch.equal(out["r"], one[1])


# -- 4. reproducibility and independence, 5. clambda[0:nC] is ignored --------------------------------------------------------------------
def test_reproducible_independent_and_head_of_clambda_ignored():
    spec, p, d = case("D8")
    a, b = run(p, d), run(p, d)
    assert torch.equal(a["res"], b["res"]) and torch.equal(a["r"], b["r"])
    alone = p.kkt(*[dev(d[k][2:3]) for k in ("x", "lo", "up", "lam")], want_residual=True)
    assert torch.equal(alone["res"][0], a["res"][2]) and torch.equal(alone["r"][0], a["r"][2])
    lam = d["lam"].copy(); lam[:, :spec.nC] = np.nan
    n = p.kkt(dev(d["x"]), dev(d["lo"]), dev(d["up"]), dev(lam), want_residual=True)
    assert torch.equal(n["res"], a["res"]) and torch.equal(n["r"], a["r"])


# -- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    spec, p, d = case("D8")
    L = api.lib()
    t = [dev(d[k]) for k in ("x", "lo", "up", "lam")]
    nb = d["x"].shape[0]
    res = torch.empty((nb, 6), dtype=torch.float64, device="cuda:0")
    st = p._stream()
    assert L.ntg_batch_kkt(p.h, nb, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, res.data_ptr(), None, st) == -2      # null d_clambda
    assert L.ntg_batch_kkt(p.h, nb, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None, None, st) == -2     # no output
    assert L.ntg_batch_kkt(p.h, nb, None, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), res.data_ptr(), None, st) == -2     # null d_x
    assert L.ntg_batch_kkt(p.h, nb, t[0].data_ptr(), None, t[2].data_ptr(), t[3].data_ptr(), res.data_ptr(), None, st) == -2     # null bounds
    assert L.ntg_batch_kkt(p.h, 0, None, None, None, None, None, None, st) == 0                                                  # empty batch
    host = api.Plan(dataclasses.replace(cf.config_O(ninterv=4), family=-1), 0)   # NTG_FAM_HOST
    lo, up = cf.obstacle_bounds(2)
    hs = host.spec
    with pytest.raises(api.NtgError, match="-4") as e:
        host.kkt(dev(np.ones((2, hs.nC))), dev(lo), dev(up), dev(np.zeros((2, hs.nC + hs.nclin + hs.ncnln))))
    assert "host-callback plans" in str(e.value)
    pf = api.Plan(cf.config_OF(3), 0)                                            # a family that needs parameters, none set
    _, lo, up = cf.obstacle_field_problems(2, 3)
    with pytest.raises(api.NtgError, match="-2"):
        pf.kkt(dev(np.ones((2, pf.spec.nC))), dev(lo), dev(up), dev(np.zeros((2, pf.spec.nC + pf.spec.nclin + pf.spec.ncnln))))


# -- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def test_solved_batch_passes_the_audit():
    """the solve of tests/test_gpu_large.py::test_reduced_grid_solve_matches_oracle for D: stationarity at that test's threshold, and
    the complementarity bound that follows from its helper's other assertions (inactive rows: |lam| <= 1e-6 max(1, lmax), slack <= 1;
    rows within 1e-5 (1 + |bound|) of a bound: slack <= that; wrong-signed multipliers <= 1e-9; linear equality rows: residual <=
    1e-9 rowscale + 1e-9, both slacks at most that)"""
    spec = cf.config_D(ninterv=8)
    p = api.Plan(spec, 0)
    nb = 6
    lo, up = cf.quadrotor_bounds(nb)
    x = torch.ones((nb, spec.nC), dtype=torch.float64, device="cuda:0")
    out = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=1), want_lambda=True)
    k = p.kkt(x, dev(lo), dev(up), out["clambda"])
    torch.cuda.synchronize()
    assert np.isin(out["inform"].cpu().numpy(), (0, 1)).all()
    res = k["res"].cpu().numpy()
    A = p.tables()["A"]; xg = x.cpu().numpy()
    nl0 = spec.nbounds - spec.nnlic - spec.nnltc - spec.nnlfc
    for i in range(nb):
        lmax = res[i, 5]
        fin = np.concatenate([lo[i, nl0:], up[i, nl0:]]); fin = np.abs(fin[np.abs(fin) < INF])
        Lmax = fin.max(initial=0.0)
        rowscale_max = (np.abs(A).max(axis=1) * max(1.0, np.abs(xg[i]).max())).max()
        bound = 1e-6 * max(1.0, lmax) + 1e-5 * (1 + Lmax) * lmax + 1e-9 + lmax * (1e-9 * rowscale_max + 1e-9)
        print(f"problem {i}: res {res[i]}  stationarity {res[i, 0] / max(1.0, res[i, 1]):.2e}  complementarity bound {bound:.2e}")
        assert res[i, 0] <= 2e-5 * max(1.0, res[i, 1]), (i, res[i])
        assert res[i, 4] <= bound, (i, res[i, 4], bound)
