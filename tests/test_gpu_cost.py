"""-m gpu: ntg_batch_cost / Plan.cost -- the running cost of trajectories at arbitrary times under any quadrature.

Reference, computed on the CPU once per case: the flat flag of every (problem, time) from the oracle's SplineInterp (orc_spline_interp,
colloc.c:449-484), the running cost L from the oracle's family function (orc_family_ucf; the host shims of tests/modules for the obstacle
field and the unicycle module), the sum  sum_i w_i L_i  in float64 with math.fsum.

Tolerances (the project's tolerance for the cost against the reference's code, VERDICT row a6, on the same arithmetic):
d_vals 1e-12 relative to max(1, |L|); d_cost 1e-12 relative to sum_i |w_i L_i|."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import orc
import family_oracle as fo
import param_oracle as po
from ntg_amd import api, configs as cf, quadrature as quad
from gpu_common import SPECS, dev
from test_gpu_grids import grids_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-12
NT = 128   # NTG_CHECK_NT: times of one tile
dp = C.POINTER(C.c_double)
UCF = C.CFUNCTYPE(None, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp, C.POINTER(dp))


def oracle_ucf(spec):
    """the oracle's running cost of a built-in family (oracle/families.c), as a callable"""
    L = orc.lib()
    L.orc_family_ucf.restype = C.c_void_p
    L.orc_family_ucf.argtypes = [C.c_int]
    ptr = L.orc_family_ucf(spec.family)
    assert ptr, "the oracle has no running cost for family %d" % spec.family
    L.orc_family_set_nout(spec.nout)
    return UCF(ptr)


def shim_ucf(cb):
    """the running cost of a host shim (family_oracle.Callbacks / param_oracle.Shim)"""
    return UCF(cb.fn["ucf"].value)


def ref_vals(spec, x, times, ucf, knots=None, bps=None):
    """L [batch][ntimes]: SplineInterp of every output at every time, then the family's running cost on that flag.  times [ntimes] or
    [batch][ntimes]; knots / bps [batch][...]: per-problem grids (every output on problem b's knots)."""
    L = orc.lib()
    x = np.asarray(x, dtype=np.float64); times = np.asarray(times, dtype=np.float64)
    nb, nt = x.shape[0], times.shape[-1]
    iC = np.concatenate([[0], np.cumsum(spec.ncoef)])
    dm = int(max(spec.maxderiv))
    z = np.zeros((spec.nout, dm)); zp = (dp * spec.nout)(*[z[o].ctypes.data_as(dp) for o in range(spec.nout)])
    df = np.zeros(spec.nz); f = C.c_double(); mode = C.c_int(0); ns = C.c_int(0)
    out = np.zeros((nb, nt))
    for b in range(nb):
        tb = times if times.ndim == 1 else times[b]
        grid = np.asarray(spec.bps if bps is None else bps[b])
        for ti in range(nt):
            for o in range(spec.nout):
                kn = np.ascontiguousarray(spec.knots[o] if knots is None else knots[b]); co = np.ascontiguousarray(x[b, iC[o]:iC[o + 1]])
                L.orc_spline_interp(z[o].ctypes.data_as(dp), C.c_double(float(tb[ti])), kn.ctypes.data_as(dp), int(spec.kninterv[o]),
                                    co.ctypes.data_as(dp), int(spec.ncoef[o]), int(spec.order[o]), int(spec.mult[o]), int(spec.maxderiv[o]))
            i = C.c_int(max(int(np.searchsorted(grid, tb[ti], side="right")) - 1, 0))   # the last breakpoint at or before the time
            mode.value = 0
            ucf(C.byref(mode), C.byref(ns), C.byref(i), C.byref(f), df.ctypes.data_as(dp), zp)
            out[b, ti] = f.value
    return out


def ref_cost(vals, weights):
    w = np.broadcast_to(np.asarray(weights), vals.shape)
    return (np.array([math.fsum(w[b] * vals[b]) for b in range(vals.shape[0])]),
            np.array([math.fsum(np.abs(w[b] * vals[b])) for b in range(vals.shape[0])]))


def compare(out, vals, weights, label=""):
    """prints every figure before it asserts"""
    ev = ec = 0.0
    if "vals" in out:
        got = out["vals"].cpu().numpy()
        assert got.shape == vals.shape
        ev = float((np.abs(got - vals) / np.maximum(1.0, np.abs(vals))).max())
    if "cost" in out:
        c, scale = ref_cost(vals, weights)
        ec = float((np.abs(out["cost"].cpu().numpy() - c) / np.maximum(scale, 1e-300)).max())
    print(f"cost {label}: vals {ev:.2e} cost {ec:.2e} (max |L| {np.abs(vals).max():.3g})")
    assert ev <= TOL and ec <= TOL


def tgrid(spec, n):
    """n uniform times over the knot range, never an ulp outside it"""
    k0 = np.asarray(spec.knots[0])
    return np.clip(np.linspace(k0[0], k0[-1], n), k0[0], k0[-1])


# ---- 1. against the solver's own objective: trapezoid nodes and weights of the plan ----
@pytest.mark.parametrize("name", ["A", "K0", "O"])
def test_trapezoid_on_the_breakpoints_is_the_objective(name):
    """kincar, vanderpol and the obstacle family have no initial or final cost: f of ntg_batch_eval is the trapezoid sum alone"""
    spec = cf.config_O(ninterv=4) if name == "O" else SPECS[name]()
    assert spec.nicf == 0 and spec.nfcf == 0 and spec.nucf == 1
    p = api.Plan(spec, 0)
    if name == "O":
        x, fgold = np.random.default_rng(2).normal(size=(5, spec.nC)), None
    else:
        g = np.load(os.path.join(GOLD, f"ref_{name}.npz"))
        x, fgold = g["x"], g["f"]
    t, w = quad.trapezoid(spec.bps)
    out = p.cost(dev(x), dev(t), dev(w), want_vals=True)
    f = p.eval(dev(x), 0)["f"].cpu().numpy()
    torch.cuda.synchronize()
    vals = ref_vals(spec, x, t, oracle_ucf(spec))
    compare(out, vals, w, name + " trapezoid")
    scale = ref_cost(vals, w)[1]
    cost = out["cost"].cpu().numpy()
    print(f"{name}: cost vs eval f {np.abs(cost - f).max():.2e} of {scale.max():.3g}")
    assert (np.abs(cost - f) <= TOL * scale).all()
    if fgold is not None:
        print(f"{name}: cost vs recorded f {np.abs(cost - fgold).max():.2e}")
        assert (np.abs(cost - fgold) <= TOL * scale).all()


# ---- 2. tile edges, and workgroups that walk over more than one problem ----
@pytest.fixture(scope="module")
def bplan():
    return api.Plan(cf.config_B(), 0)


@pytest.fixture(scope="module")
def bref(bplan):
    """7 coefficient rows and their running cost at 300 times, computed once: the cases below take their times from these 300"""
    spec = bplan.spec
    x = np.random.default_rng(5).normal(size=(7, spec.nC))
    times = tgrid(spec, 300)
    return x, times, ref_vals(spec, x, times, oracle_ucf(spec))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("ntimes", [1, 63, 127, 128, 129, 300])
def test_tile_edges(bplan, bref, ntimes, batch):
    x, times, vals = bref
    sel = np.array([137]) if ntimes == 1 else np.arange(ntimes)
    w = np.random.default_rng(ntimes).uniform(-0.5, 1.5, sel.size)   # any weights, of both signs
    out = bplan.cost(dev(x[:batch]), dev(times[sel]), dev(w), want_vals=True)
    torch.cuda.synchronize()
    compare(out, vals[:batch][:, sel], w, f"B ntimes {ntimes} batch {batch}")


def test_a_workgroup_walks_over_several_problems(bplan, bref):
    """the launcher's rule (time_tile_walk): gridDim.y = min(batch, max(1, ceil(8 ncu / ntiles))).  One problem more than that at the
    largest ntimes of this file, so that the first group's workgroups take two problems; the problems repeat 7 coefficient rows in a
    random order (a wrong problem index would show in 6 cases of 7)"""
    x7, times, v7 = bref
    ntiles = (times.size + NT - 1) // NT
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    groups = max(1, (8 * ncu + ntiles - 1) // ntiles)
    batch = groups + 1
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 7, batch)
    w = rng.uniform(0.0, 1.0, times.size)
    out = bplan.cost(dev(x7[idx]), dev(times), dev(w), want_vals=True)
    torch.cuda.synchronize()
    print(f"ncu {ncu} tiles {ntiles} groups {groups} batch {batch}")
    compare(out, v7[idx], w, f"B walk, batch {batch}")


# ---- 3. every family's instance ----
@pytest.fixture(scope="module")
def fams():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    ids = {m: api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", m + ".hip"))) for m in ("unicycle", "tracking")}
    ids["cb"] = fo.Callbacks(fo.build_shim("unicycle_host"), "uni_")
    return ids


@pytest.mark.parametrize("name", ["T", "A", "D8", "E8"])
def test_builtin_families(name):
    """testfam (all six slots: the initial and final cost must not be in the result), vanderpol, quadrotor, manipulator"""
    spec, nb = SPECS[name](), 3
    p = api.Plan(spec, 0)
    x = np.random.default_rng(11).normal(size=(nb, spec.nC))
    t, w = quad.gauss_legendre(spec.knots[0], 3)
    out = p.cost(dev(x), dev(t), dev(w), want_vals=True)
    torch.cuda.synchronize()
    vals = ref_vals(spec, x, t, oracle_ucf(spec))
    compare(out, vals, w, name)
    if name == "T":
        assert spec.nicf == 1 and spec.nfcf == 1
        tt, tw = quad.trapezoid(spec.bps)
        c = p.cost(dev(x), dev(tt), dev(tw))["cost"].cpu().numpy()
        f = p.eval(dev(x), 0)["f"].cpu().numpy()
        assert (np.abs(f - c) > 1e-3).all()   # what the two other cost functions contribute


def test_obstacle_field_with_per_problem_parameters():
    spec, nb = cf.config_OF(3, ninterv=4), 4
    prm, _, _ = cf.obstacle_field_problems(nb, 3)
    p = api.Plan(spec, 0)
    p.set_params(dev(prm))
    shim = po.Shim("obstacle_field_host")
    shim.set_problem(spec, prm[0])
    x = np.random.default_rng(12).normal(size=(nb, spec.nC))
    t, w = quad.gauss_legendre(spec.knots[0], 2)
    out = p.cost(dev(x), dev(t), dev(w), want_vals=True)
    torch.cuda.synchronize()
    compare(out, ref_vals(spec, x, t, shim_ucf(shim)), w, "OF")   # (the family's running cost does not read the parameters)


def test_unicycle_module(fams):
    spec, nb = cf.config_U(fams["unicycle"]), 4
    p = api.Plan(spec, 0)
    x = np.random.default_rng(13).normal(size=(nb, spec.nC))
    t, w = quad.gauss_legendre(spec.knots[0], 3)
    out = p.cost(dev(x), dev(t), dev(w), want_vals=True)
    torch.cuda.synchronize()
    compare(out, ref_vals(spec, x, t, shim_ucf(fams["cb"])), w, "unicycle")


def test_tracking_module_is_refused(fams):
    spec, nb = cf.config_TR(fams["tracking"]), 4
    p = api.Plan(spec, 0)
    prm, _, _ = cf.tracking_problems(spec, nb)
    p.set_params(dev(prm))
    t, w = quad.trapezoid(spec.bps)
    with pytest.raises(api.NtgError, match="-4"):   # NTG_E_UNSUPPORTED: its data exists at breakpoints only
        p.cost(dev(np.ones((nb, spec.nC))), dev(t), dev(w))


# ---- 4. per-problem grids ----
def _debug_cost(plan, x, times, weights, stride, cap):
    """ntg_debug_batch_cost: ntg_batch_cost with the scratch cap of the per-problem time tables stated (forces several chunks)"""
    L = api.lib()
    L.ntg_debug_batch_cost.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_longlong]
    nb, nt = x.shape[0], times.shape[-1]
    cost = torch.zeros(nb, dtype=torch.float64, device=x.device); vals = torch.zeros((nb, nt), dtype=torch.float64, device=x.device)
    rc = L.ntg_debug_batch_cost(plan.h, nb, x.data_ptr(), nt, times.data_ptr(), weights.data_ptr(), stride, cost.data_ptr(), vals.data_ptr(), None, cap)
    assert rc == 0, L.ntg_last_error().decode()
    torch.cuda.synchronize()
    return dict(cost=cost, vals=vals)


def test_per_problem_grids():
    """3 problems with different horizons: shared times (stride 0) and every problem's own Gauss nodes (stride ntimes)"""
    spec, nb = cf.config_O(ninterv=4), 3
    knots, bps = grids_for(spec, nb, warp=0.2)
    assert len({float(k[-1]) for k in knots}) == nb
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    x = np.random.default_rng(6).normal(size=(nb, spec.nC))
    ucf = oracle_ucf(spec)
    t, w = quad.gauss_legendre(knots, 4)
    assert t.shape == (nb, 16)
    own = p.cost(dev(x), dev(t), dev(w), want_vals=True)
    sh_t, sh_w = quad.gauss_legendre(np.linspace(0.0, knots[:, -1].min(), 34), 4)   # 132 times inside every problem's knot range: two tiles
    sh = p.cost(dev(x), dev(sh_t), dev(sh_w), want_vals=True)
    torch.cuda.synchronize()
    compare(own, ref_vals(spec, x, t, ucf, knots, bps), w, "grids, own Gauss nodes")
    compare(sh, ref_vals(spec, x, sh_t, ucf, knots, bps), sh_w, "grids, shared times")
    # the batch in chunks of one problem: bit for bit the one-chunk result
    a = _debug_cost(p, dev(x), dev(t), dev(w), 16, 1)
    b = _debug_cost(p, dev(x), dev(sh_t), dev(sh_w), 0, 1)
    assert all(torch.equal(a[k], own[k]) for k in own) and all(torch.equal(b[k], sh[k]) for k in sh)
    with pytest.raises(api.NtgError, match="-2"):   # the grids are for exactly this batch
        p.cost(dev(x[:2]), dev(sh_t), dev(sh_w))
    p.clear_grids()


# ---- 5. determinism ----
def test_results_are_bit_identical(bplan, bref):
    x7, times, _ = bref
    w = np.random.default_rng(3).uniform(0.0, 1.0, times.size)
    xd, td, wd = dev(x7[:3]), dev(times), dev(w)
    a = bplan.cost(xd, td, wd, want_vals=True)
    b = bplan.cost(xd, td, wd, want_vals=True)
    assert all(torch.equal(a[k], b[k]) for k in a)                                  # call to call
    one = bplan.cost(xd[1:2].contiguous(), td, wd, want_vals=True)
    assert all(torch.equal(one[k][0], a[k][1]) for k in a)                          # problem 1 alone
    few = bplan.cost(xd, td[:64].contiguous(), wd[:64].contiguous(), want_vals=True)
    assert torch.equal(few["vals"], a["vals"][:, :64])                              # ntimes 64 or 300: the same 64 values


# ---- 6. the audit sees what it is for ----
def test_gauss_converges_where_the_trapezoid_sum_is_off():
    """Family: kincar (families.hpp, NTG_FAM_KINCAR), L = sum_o (z_o'')^2: a polynomial in the flag.  On a knot interval z_o is a polynomial
    of degree order - 1, its second derivative of degree order - 3, L of degree 2 (order - 3): Gauss-Legendre with npts nodes per knot
    interval is exact once 2 npts - 1 >= 2 (order - 3).  So npts and npts + 2 must agree to the d_cost tolerance, while the plan's own
    trapezoid sum on a coarse breakpoint grid -- the objective its solver minimised -- is off by far more than 100 x that."""
    ncars, order, mult, ninterv, nbps = 1, 6, 3, 4, 9   # two breakpoint intervals per knot interval
    spec = cf._kincar_spec(ncars, order, mult, ninterv, nbps, 5.0, "kincar-coarse-bps")
    nb = 4
    p = api.Plan(spec, 0)
    lo, up = cf.kincar_random_bounds(ncars, nb)
    x = dev(np.ones((nb, spec.nC)))
    sol = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=1))
    assert (sol["inform"].cpu().numpy() == 0).all()
    deg = 2 * (order - 1 - 2)   # piecewise degree of the integrand: the cost reads derivative 2 (tcostav) of splines of degree order - 1
    assert all(d == 2 for _, d in spec.tcostav) and max(spec.maxderiv) == 3
    npts = (deg + 2) // 2       # the smallest npts with 2 npts - 1 >= deg
    assert 2 * npts - 1 >= deg > 2 * (npts - 1) - 1
    res = {}
    for n in (npts, npts + 2):
        t, w = quad.gauss_legendre(spec.knots[0], n)
        out = p.cost(x, dev(t), dev(w), want_vals=True)
        res[n] = out["cost"].cpu().numpy()
        scale = (np.abs(w)[None, :] * np.abs(out["vals"].cpu().numpy())).sum(axis=1)
    tt, tw = quad.trapezoid(spec.bps)
    trap = p.cost(x, dev(tt), dev(tw))["cost"].cpu().numpy()
    obj = sol["objective"].cpu().numpy()
    print("gauss", res[npts], "\ngauss + 2", res[npts + 2], "\ntrapezoid", trap, "\nobjective", obj, "\nscale", scale)
    assert (np.abs(res[npts] - res[npts + 2]) <= TOL * scale).all()
    assert (np.abs(trap - res[npts]) > 100 * TOL * scale).all()


# ---- 7. refusals and degenerate calls ----
def test_refusals_and_degenerate_calls(bplan):
    spec, nb = bplan.spec, 4
    x = dev(np.ones((nb, spec.nC)))
    tt, tw = quad.trapezoid(tgrid(spec, 9))
    t, w = dev(tt), dev(tw)
    L, st = api.lib(), None
    cost = torch.full((nb,), 7.0, dtype=torch.float64, device="cuda:0")
    raw = lambda plan, batch, nt, stride, xp, tp, wp, c, v: L.ntg_batch_cost(plan.h, batch, xp, nt, tp, wp, stride, c, v, st)
    X, T, W, Cc = x.data_ptr(), t.data_ptr(), w.data_ptr(), cost.data_ptr()
    assert raw(bplan, 0, 9, 0, X, T, W, Cc, None) == 0 and raw(bplan, nb, 0, 0, X, T, W, Cc, None) == 0
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == 7.0).all()                       # nothing ran
    assert raw(bplan, nb, 9, 0, None, T, W, Cc, None) == -2        # null d_x
    assert raw(bplan, nb, 9, 0, X, None, W, Cc, None) == -2        # null d_times
    assert raw(bplan, nb, 9, 0, X, T, W, None, None) == -2         # both outputs null
    assert raw(bplan, nb, 9, 0, X, T, None, Cc, None) == -2        # d_cost without weights
    assert "weights" in L.ntg_last_error().decode()
    assert raw(bplan, nb, 9, 5, X, T, W, Cc, None) == -2           # times_stride < ntimes
    assert raw(bplan, nb, 9, 9, X, T, W, Cc, None) == -2           # per-problem times without per-problem grids
    assert "per-problem grids" in L.ntg_last_error().decode()
    with pytest.raises(api.NtgError):
        bplan.cost(x, dev(np.zeros((nb, 9))), dev(np.zeros((nb, 9))))
    # values alone need no weights
    vals = torch.zeros((nb, 9), dtype=torch.float64, device="cuda:0")
    assert raw(bplan, nb, 9, 0, X, T, None, None, vals.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(vals, bplan.cost(x, t, w, want_vals=True)["vals"]) and torch.equal(vals, bplan.cost(x, t, None, want_vals=True)["vals"])
    tspec = dataclasses.replace(cf.config_T(), nucf=0)                              # initial and final cost, no running cost
    nocost = api.Plan(tspec, 0)
    tq = quad.trapezoid(tspec.bps)
    with pytest.raises(api.NtgError, match="no running cost"):
        nocost.cost(dev(np.ones((nb, tspec.nC))), dev(tq[0]), dev(tq[1]))
    host = api.Plan(dataclasses.replace(cf.config_B(), family=-1), 0)               # NTG_FAM_HOST
    with pytest.raises(api.NtgError, match="-4") as e:
        host.cost(x, t, w)
    assert "host-callback plans" in str(e.value)
    of = api.Plan(cf.config_OF(3, ninterv=4), 0)                                    # parameters: not set, then set for another batch
    prm, _, _ = cf.obstacle_field_problems(nb, 3)
    xf = dev(np.ones((nb, of.spec.nC)))
    with pytest.raises(api.NtgError, match="-2"):
        of.cost(xf, t, w)
    of.set_params(dev(prm))
    assert of.cost(xf, t, w)["cost"].shape == (nb,)
    with pytest.raises(api.NtgError, match="-2"):
        of.cost(xf[:2].contiguous(), t, w)
