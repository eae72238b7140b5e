"""-m gpu: per-problem grids (ntg_plan_set_grids) on plans with linear inequality rows (ntg_spec.lin_ineq): the values of the range rows
on every grid (grids.hip, grid_ilin_kernel), read back through Plan.grid_tables, and the augmented-Lagrangian solve on those grids, each
problem against the oracle built on that problem's grid (it reads ranges from the bounds, as NPSOL does).

Tolerances: the grid's A 1e-13 relative to its row; solves as tests/test_gpu_linineq.py (objective 1e-7 relative for the end-state
windows, 1e-6 for trajectory rows and all-range plans; x 1e-5 relative; equality rows 1e-8, ranges 1e-7)."""
import numpy as np
import pytest
import torch

import orc
from ntg_amd import api, configs as cf
from gpu_common import dev, rel
from test_gpu_grids import grids_for, spec_on
from test_gpu_linineq import _bounds, _spec

pytestmark = pytest.mark.gpu

WINDOWS = [0] * 6 + [0, 0, 0, 1, 0, 1]   # y(T) and y''(T) in ranges (test_gpu_linineq._bounds)


def _ceiling_spec(base):
    """base plus one linear trajectory row on y declared a range: a ceiling at every breakpoint (bounds column 6)"""
    spec = base
    ltc = np.zeros((1, spec.nz)); ltc[0, 3] = 1.0
    spec.ltc = ltc
    spec.lin_ineq = [0] * 6 + [1] + [0] * 6
    return spec


def _with_ceiling(lo, up, ymax):
    nb = lo.shape[0]
    lo = np.concatenate([lo[:, :6], np.full((nb, 1), -cf.INF_BOUND), lo[:, 6:]], axis=1)
    up = np.concatenate([up[:, :6], np.broadcast_to(np.asarray(ymax, dtype=np.float64).reshape(-1, 1), (nb, 1)), up[:, 6:]], axis=1)
    return lo, up


def _grids(name, nb, seed):
    spec = _spec(name, list(WINDOWS))
    knots, bps = grids_for(spec, nb, warp=0.3 if name == "K0" else 0.2, seed=seed)
    return spec, knots, bps


def _check_tables(p, spec, knots, bps):
    for b in range(knots.shape[0]):
        ref = orc.export_tables(spec_on(spec, knots[b], bps[b]))
        got = p.grid_tables(b)
        scale = np.maximum(np.abs(ref["A"]).max(axis=1, keepdims=True), 1e-300)
        assert (np.abs(got["A"] - ref["A"]) <= 1e-13 * scale).all(), b
        assert rel(got["blk"], ref["blk"]) <= 1e-12, b
        assert np.array_equal(got["off"], ref["off"])


@pytest.mark.parametrize("name", ["K0", "B"])
def test_set_grids_with_range_rows_and_their_values(name):
    """set_grids used to refuse any plan with inequality rows; now every problem's A (equality and range rows) is the oracle's on its grid"""
    nb = 12
    spec, knots, bps = _grids(name, nb, seed=17)
    p = api.Plan(spec, 0)
    A0 = p.tables()["A"]
    p.set_grids(dev(knots), dev(bps), with_precond=True)
    _check_tables(p, spec, knots, bps)
    assert np.abs(p.grid_tables(0)["A"] - p.grid_tables(1)["A"]).max() > 1e-3      # the grids do differ
    np.testing.assert_array_equal(p.tables()["A"], A0)                              # tables() stays the plan's own grid


def _check_solution(spec, sb, lo, up, xg, obj, inf, lam, ref, flags, otol):
    assert ref["inform"] in (0, 1) and inf in (0, 1)
    assert abs(obj - ref["objective"]) <= otol * max(1.0, abs(ref["objective"]))
    assert np.abs(xg - ref["x"]).max() <= 1e-5 * np.abs(ref["x"]).max()
    tab = orc.export_tables(sb, lo, up)
    A = tab["A"]
    Ax = A @ xg
    nl = spec.nclin
    lo, up = tab["bl"][spec.nC:spec.nC + nl], tab["bu"][spec.nC:spec.nC + nl]   # bounds of every linear row (a trajectory row's at each breakpoint)
    eq = [r for r in range(nl) if not flags[r]]; iq = [r for r in range(nl) if flags[r]]
    if eq:
        assert np.abs(Ax[eq] - lo[eq]).max() <= 1e-8 * max(1.0, np.abs(A[eq]).max())
    assert (Ax[iq] >= lo[iq] - 1e-7).all() and (Ax[iq] <= up[iq] + 1e-7).all()
    if lam is None:
        return False
    # multiplier sign and complementarity on the range rows (NPSOL's layout [coefficients; linear rows; nonlinear rows])
    ll = lam[spec.nC:spec.nC + nl]
    for r in iq:
        at_lo, at_up = Ax[r] <= lo[r] + 1e-6, Ax[r] >= up[r] - 1e-6
        assert (ll[r] >= -1e-8 if at_lo else True) and (ll[r] <= 1e-8 if at_up else True)
        assert abs(ll[r]) <= 1e-6 * max(1.0, np.abs(ll).max()) or at_lo or at_up
    return bool((np.abs(ll[iq]) > 1e-8).any())


@pytest.mark.parametrize("name", ["K0", "B"])
@pytest.mark.parametrize("hessian", [0, 1])
def test_end_state_windows_on_per_problem_horizons(name, hessian):
    nb = 8
    spec, knots, bps = _grids(name, nb, seed=17)
    lo, up = _bounds(name, nb)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=bool(hessian))
    assert p.solve_kernel(nb, api.default_opts(hessian=hessian)) == "sqp_kernel"
    x = dev(np.ones((nb, spec.nC)))
    out = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=hessian, itlim=3000), want_lambda=True)
    torch.cuda.synchronize()
    inf = out["inform"].cpu().numpy(); obj = out["objective"].cpu().numpy(); lam = out["clambda"].cpu().numpy(); xg = x.cpu().numpy()
    nact = 0
    for b in range(nb):
        sb = spec_on(spec, knots[b], bps[b])
        ref = orc.solve_one(sb, lo[b], up[b], np.ones(spec.nC), orc.default_opts(hessian=hessian, itlim=3000))
        nact += _check_solution(spec, sb, lo[b], up[b], xg[b], obj[b], inf[b], lam[b], ref, WINDOWS, 1e-7)
    assert nact >= 2                                   # the windows bind for some of the problems


def _ceiling_problem(nb, seed):
    spec = _ceiling_spec(cf.config_B())
    knots, bps = grids_for(spec, nb, warp=0.2, seed=seed)
    lo0, up0 = cf.kincar_random_bounds(1, nb)
    ymax = np.maximum(lo0[:, 3], lo0[:, 9]) + 0.05           # a ceiling just above both end points
    lo, up = _with_ceiling(lo0, up0, ymax)
    return spec, knots, bps, lo, up, ymax


def test_trajectory_ceiling_on_per_problem_horizons():
    """101 range rows (y(t_i) <= ymax at every breakpoint) on 8 horizons, hessian = 1: every problem is the oracle's on its grid, stays under
    its ceiling, at least two touch it, and the optima are not those of the shared grid"""
    nb = 8
    spec, knots, bps, lo, up, ymax = _ceiling_problem(nb, seed=21)
    P = spec.nbps
    flags = [0] * 6 + [1] * P + [0] * 6
    opts = api.default_opts(hessian=1, itlim=3000)
    p = api.Plan(spec, 0)
    xs = dev(np.ones((nb, spec.nC)))
    p.solve(dev(lo), dev(up), xs, opts)                      # the shared grid, same bounds
    p.set_grids(dev(knots), dev(bps), with_precond=True)
    _check_tables(p, spec, knots, bps)
    x = dev(np.ones((nb, spec.nC)))
    out = p.solve(dev(lo), dev(up), x, opts)
    torch.cuda.synchronize()
    inf = out["inform"].cpu().numpy(); obj = out["objective"].cpu().numpy(); xg = x.cpu().numpy()
    nact = 0
    for b in range(nb):
        sb = spec_on(spec, knots[b], bps[b])
        ref = orc.solve_one(sb, lo[b], up[b], np.ones(spec.nC), orc.default_opts(hessian=1, itlim=3000))
        _check_solution(spec, sb, lo[b], up[b], xg[b], obj[b], inf[b], None, ref, flags, 1e-6)
        y = (p.grid_tables(b)["A"] @ xg[b])[6:6 + P]
        assert y.max() <= ymax[b] + 1e-6
        nact += int(y.max() >= ymax[b] - 1e-6)
    assert nact >= 2
    assert np.abs(xg - xs.cpu().numpy()).max() > 1e-3


def test_every_linear_row_a_range_on_per_problem_horizons():
    """mE = 0: no equality row, so grid_lin_kernel does not run and nothing is projected; the range rows' values still come per grid.
    (Mode 0: the cost model of kincar is singular without pinned coefficients, so this plan has no preconditioner on any grid.)"""
    flags = [1] * 12
    spec = _spec("K0", flags)
    nb = 4
    lo0, up0 = cf.bounds_K0_shipped()
    lo = np.tile(lo0, (nb, 1)) - 0.05 * (1 + np.arange(nb))[:, None]
    up = np.tile(up0, (nb, 1)) + 0.05 * (1 + np.arange(nb))[:, None]
    knots, bps = grids_for(spec, nb, warp=0.3, seed=23)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    _check_tables(p, spec, knots, bps)
    x = dev(np.ones((nb, spec.nC)))
    out = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=0, itlim=3000))
    torch.cuda.synchronize()
    inf = out["inform"].cpu().numpy(); obj = out["objective"].cpu().numpy(); xg = x.cpu().numpy()
    for b in range(nb):
        sb = spec_on(spec, knots[b], bps[b])
        ref = orc.solve_one(sb, lo[b], up[b], np.ones(spec.nC), orc.default_opts(hessian=0, itlim=3000))
        _check_solution(spec, sb, lo[b], up[b], xg[b], obj[b], inf[b], None, ref, flags, 1e-6)


def test_obstacle_and_ceiling_rows_together():
    """config O (a nonlinear obstacle row at every breakpoint) plus a linear ceiling on y declared a range: the generic sqp_kernel instance
    with both kinds of augmented-Lagrangian rows, on the shared grid and on 8 horizons, against the oracle in mode 1.  hessian = 3 acts as
    1 on such a plan (no band model with inequality rows): the same bits."""
    nb = 8
    spec = _ceiling_spec(cf.config_O())
    lo0, up0 = cf.obstacle_bounds(nb)
    lo, up = _with_ceiling(lo0, up0, 4.0)
    knots, bps = grids_for(spec, nb, warp=0.2, seed=9)
    flags = [0] * 6 + [1] * spec.nbps + [0] * 6
    p = api.Plan(spec, 0)
    for grid in (False, True):
        if grid:
            p.set_grids(dev(knots), dev(bps), with_precond=True)
        res = []
        for hess in (1, 3):
            assert p.solve_kernel(nb, api.default_opts(hessian=hess)) == "sqp_kernel"
            x = dev(np.ones((nb, spec.nC)))
            out = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=hess, itlim=3000))
            torch.cuda.synchronize()
            res.append((x.cpu().numpy(), out["objective"].cpu().numpy(), out["inform"].cpu().numpy()))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        xg, obj, inf = res[0]
        for b in range(nb):
            sb = spec_on(spec, knots[b], bps[b]) if grid else spec
            ref = orc.solve_one(sb, lo[b], up[b], np.ones(spec.nC), orc.default_opts(hessian=1, itlim=3000))
            _check_solution(spec, sb, lo[b], up[b], xg[b], obj[b], inf[b], None, ref, flags, 1e-6)
            zr = orc.eval_batch(sb, xg[b][None], 2)
            assert zr["c"][0].min() >= lo[b][-1] - 1e-6 * lo[b][-1]          # outside the obstacle


def test_grid_with_weight_outside_the_range_rows_pattern_is_refused():
    """Breakpoint 5 sits exactly on knot 1, where the y value of the basis function starting there is an exact zero of the plan's pattern.
    Moved inside the same knot interval, the ceiling row at that breakpoint gets weight there: refused, naming the problem and the row,
    before anything is solved (the rule the equality rows follow)."""
    nb = 4
    spec, knots, bps, lo, up, ymax = _ceiling_problem(nb, seed=21)
    assert spec.bps[5] == spec.knots[0][1] and bps[2, 5] == knots[2, 1]
    bad = bps.copy()
    bad[2, 5] = knots[2, 1] + 0.3 * (knots[2, 2] - knots[2, 1])
    p = api.Plan(spec, 0)
    with pytest.raises(api.NtgError, match=r"outside the plan's sparsity pattern \(problem 2, linear row 11"):
        p.set_grids(dev(knots), dev(bad), with_precond=True)
    assert p.grid_batch == 0
    p.set_grids(dev(knots), dev(bps), with_precond=True)      # the unmoved grids are fine
    assert p.grid_batch == nb


def test_batch_handling_and_life_cycle():
    nb = 8
    spec, knots, bps = _grids("K0", nb, seed=17)
    lo, up = _bounds("K0", nb)
    opts = api.default_opts(hessian=1, itlim=3000)
    p = api.Plan(spec, 0)
    for bad in (-1, 0):
        with pytest.raises(api.NtgError):             # no grids set
            p.grid_tables(bad)
    x0 = dev(np.ones((nb, spec.nC)))
    o0 = p.solve(dev(lo), dev(up), x0, opts)
    shared = (x0.cpu().numpy().copy(), o0["objective"].cpu().numpy().copy())
    p.set_grids(dev(knots), dev(bps), with_precond=True)
    with pytest.raises(api.NtgError):
        p.grid_tables(nb)
    with pytest.raises(api.NtgError):
        p.grid_tables(-1)
    x = dev(np.ones((nb, spec.nC)))
    full = p.solve(dev(lo), dev(up), x, opts)
    torch.cuda.synchronize()
    xfull, ofull = x.cpu().numpy().copy(), full["objective"].cpu().numpy().copy()
    Afull = [p.grid_tables(b)["A"] for b in range(nb)]
    with pytest.raises(api.NtgError):                 # the grids are for exactly this batch
        p.eval(dev(np.ones((3, spec.nC))))
    with pytest.raises(api.NtgError):
        p.solve(dev(lo[:3]), dev(up[:3]), dev(np.ones((3, spec.nC))), opts)
    # a subset of the grids: the same problems give the same bits
    sub = [1, 4, 6]
    p.set_grids(dev(knots[sub]), dev(bps[sub]), with_precond=True)
    xs = dev(np.ones((len(sub), spec.nC)))
    os_ = p.solve(dev(lo[sub]), dev(up[sub]), xs, opts)
    torch.cuda.synchronize()
    assert np.array_equal(xs.cpu().numpy(), xfull[sub]) and np.array_equal(os_["objective"].cpu().numpy(), ofull[sub])
    for j, b in enumerate(sub):
        assert np.array_equal(p.grid_tables(j)["A"], Afull[b])
    # back on the plan's grid: the shared solve as before set_grids
    p.clear_grids()
    with pytest.raises(api.NtgError):
        p.grid_tables(0)
    x2 = dev(np.ones((nb, spec.nC)))
    o2 = p.solve(dev(lo), dev(up), x2, opts)
    torch.cuda.synchronize()
    assert np.array_equal(x2.cpu().numpy(), shared[0]) and np.array_equal(o2["objective"].cpu().numpy(), shared[1])
    assert np.abs(xfull - shared[0]).max() > 1e-3


def test_receding_horizon_with_ceiling_on_per_problem_grids():
    """solve -> mpc_shift step by step on per-problem horizons with the ceiling row, cold re-solves (warm_start = 0), each against the oracle on
    that problem's grid; ntg_batch_mpc_run (the captured graph reading the plan's per-problem buffers) reproduces the iterates"""
    from test_gpu_mpc import shift_numpy
    nb, nsteps = 5, 3
    spec = _ceiling_spec(cf.config_B())
    knots, bps = grids_for(spec, nb, warp=0.0, seed=13)     # uniform knots per problem (the coefficient shift assumes them), horizons differ
    lo0, up0 = cf.kincar_random_bounds(1, nb)
    ymax = np.maximum(lo0[:, 3], lo0[:, 9]) + 0.05
    lo, up = _with_ceiling(lo0, up0, ymax)
    flags = [0] * 6 + [1] * spec.nbps + [0] * 6
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=True)
    specs = [spec_on(spec, knots[b], bps[b]) for b in range(nb)]
    tabs = [orc.export_tables(sb) for sb in specs]
    x = dev(np.ones((nb, spec.nC))); lo_d, up_d = dev(lo), dev(up)
    x2 = x.clone(); lo2, up2 = lo_d.clone(), up_d.clone()
    opts = api.default_opts(hessian=1, itlim=3000)
    opts.warm_start = 0
    for step in range(nsteps):
        lo_h, up_h, x_h = lo_d.cpu().numpy(), up_d.cpu().numpy(), x.cpu().numpy()
        out = p.solve(lo_d, up_d, x, opts)
        torch.cuda.synchronize()
        xg = x.cpu().numpy(); obj = out["objective"].cpu().numpy(); inf = out["inform"].cpu().numpy()
        for b in range(nb):
            ref = orc.solve_one(specs[b], lo_h[b], up_h[b], x_h[b], orc.default_opts(hessian=1, itlim=3000))
            _check_solution(spec, specs[b], lo_h[b], up_h[b], xg[b], obj[b], inf[b], None, ref, flags, 1e-6)
        exp = [shift_numpy(specs[b], tabs[b], xg[b], lo_h[b], up_h[b], 5, 1) for b in range(nb)]
        p.mpc_shift(x, lo_d, up_d, 5, 1)
        np.testing.assert_allclose(x.cpu().numpy(), np.stack([e[0] for e in exp]), rtol=0, atol=0)
        np.testing.assert_allclose(lo_d.cpu().numpy(), np.stack([e[1] for e in exp]), rtol=1e-13, atol=1e-12)
    p.mpc_run(x2, lo2, up2, nsteps, 5, 1, opts)
    torch.cuda.synchronize()
    np.testing.assert_allclose(x2.cpu().numpy(), x.cpu().numpy(), rtol=0, atol=1e-9 * max(1.0, float(x.abs().max())))
