"""-m gpu: ntg_batch_check / Plan.check -- the trajectory rows of solved problems BETWEEN the breakpoints.

Reference for row values: the oracle as it stands, on a copy of the spec whose breakpoints are the check times (same knots):
orc.eval_batch(fine, x, mode=0)["c"] gives the nonlinear trajectory rows constraint-major x time through the oracle's own collocation
and callbacks, the ltc block of orc.export_tables(fine)["A"] times x the linear ones.  Violations and `where` are numpy on those.

Tolerance: the project's evaluation tolerance, 1e-12 max|ref rows| absolute, for the rows and -- a violation is a bound minus a row
value, so it inherits the row's absolute error -- for viol.  `where` is accepted when the reference violation at the reported
(row, time) is within that tolerance of the reference maximum (robust to near-ties); in the constructed exact tie it must be the first."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

import orc
import family_oracle as fo
from ntg_amd import api, configs as cf
from gpu_common import SPECS, dev, rel
from test_gpu_grids import grids_for, spec_on

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = cf.INF_BOUND
TOL = 1e-12


def tgrid(spec, n, t1=None):
    """n uniform times over the knot range (or up to t1), never an ulp outside it"""
    k0 = np.asarray(spec.knots[0])
    return np.clip(np.linspace(k0[0], k0[-1] if t1 is None else t1, n), k0[0], k0[-1])


def traj_slots(spec):
    """bound slots of the trajectory row functions, linear first (order lic, ltc, lfc, nlic, nltc, nlfc)"""
    n0 = spec.nlic + spec.nltc + spec.nlfc + spec.nnlic
    return list(range(spec.nlic, spec.nlic + spec.nltc)) + list(range(n0, n0 + spec.nnltc))


def ref_rows(spec, x, times, cb=None):
    """[batch][nltc + nnltc][ntimes] from the oracle on the fine spec (the times sorted, with both ends of the knot range: the oracle
    sees an ordinary grid whatever the times are)"""
    x = np.asarray(x); times = np.asarray(times)
    k0 = np.asarray(spec.knots[0])
    grid = np.unique(np.concatenate([times, [k0[0], k0[-1]]]))
    idx = np.searchsorted(grid, times)
    fine = dataclasses.replace(spec, bps=grid)
    P, nb = len(grid), x.shape[0]
    out = np.zeros((nb, spec.nltc + spec.nnltc, len(times)))
    if spec.nnltc:
        if cb is None:
            c = orc.eval_batch(fine, x, mode=0)["c"]
        else:
            zero = np.zeros(spec.nbounds)
            c = np.zeros((nb, fine.ncnln))
            for b in range(nb):
                pr = fo.Problem(fine, cb, zero, zero)
                c[b] = pr.eval(x[b], mode=0)["c"]
                pr.close()
        out[:, spec.nltc:] = c[:, spec.nnlic:spec.nnlic + spec.nnltc * P].reshape(nb, spec.nnltc, P)[:, :, idx]
    if spec.nltc:
        A = orc.export_tables(fine)["A"][spec.nlic:spec.nlic + spec.nltc * P]
        out[:, :spec.nltc] = (x @ A.T).reshape(nb, spec.nltc, P)[:, :, idx]
    return out


def violations(spec, rows, lo, up):
    """max(l - c, c - u, 0) per (problem, row, time); a bound with |.| >= 1e20 is absent"""
    s = traj_slots(spec)
    l = np.asarray(lo)[:, s][:, :, None]; u = np.asarray(up)[:, s][:, :, None]
    v = np.zeros_like(rows)
    v = np.where(np.abs(l) < INF, np.maximum(v, l - rows), v)
    v = np.where(np.abs(u) < INF, np.maximum(v, rows - u), v)
    return v


def compare(spec, out, rows_ref, lo, up, label=""):
    """rows, viol and where of a Plan.check result against the reference rows; prints every figure before it asserts"""
    scale = max(np.abs(rows_ref).max(), 1e-300)
    vref = violations(spec, rows_ref, lo, up)
    nb, nt = rows_ref.shape[0], rows_ref.shape[2]
    viol = out["viol"].cpu().numpy(); where = out["where"].cpu().numpy()
    erow = np.abs(out["rows"].cpu().numpy() - rows_ref).max() / scale if "rows" in out else 0.0
    vmax = vref.reshape(nb, -1).max(axis=1)
    eviol = np.abs(viol - vmax).max() / scale
    print(f"check {label}: rows {erow:.2e} viol {eviol:.2e} of max|ref| {scale:.3g}; viol max {viol.max():.4g}")
    assert erow <= TOL and eviol <= TOL
    for b in range(nb):
        r, t = where[b]
        if viol[b] == 0.0:
            assert (r, t) == (-1, -1) and vmax[b] <= TOL * scale
        else:
            assert 0 <= r < rows_ref.shape[1] and 0 <= t < nt
            assert vref[b, r, t] >= vmax[b] - TOL * scale, (b, r, t, vref[b, r, t], vmax[b])
    return vref


def rand_bounds(spec, nb, rows_ref, seed=3):
    """two-sided bounds on the trajectory rows around the middle of what the rows take, tight enough that most problems violate"""
    rng = np.random.default_rng(seed)
    lo = np.zeros((nb, spec.nbounds)); up = np.zeros((nb, spec.nbounds))
    for j, s in enumerate(traj_slots(spec)):
        mid = np.median(rows_ref[:, j], axis=1); w = rows_ref[:, j].std(axis=1) + 1e-3
        lo[:, s] = mid - rng.uniform(0.2, 3.0, nb) * w; up[:, s] = mid + rng.uniform(0.2, 3.0, nb) * w
        if rows_ref.shape[2] == 1:   # a single time: a unit window beside the value, above it for even problems, below it for odd ones
            sh = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0)
            lo[:, s] = mid + sh - 0.5; up[:, s] = mid + sh + 0.5
    return lo, up


# ---- 1. times = the plan's breakpoints: the rows are Plan.eval's c ----
def _case(name):
    if name == "O":
        spec = cf.config_O(ninterv=4); nb = 8
        return spec, nb, None, cf.obstacle_bounds(nb)
    if name == "OF":
        spec = cf.config_OF(3, ninterv=4); nb = 8
        prm, lo, up = cf.obstacle_field_problems(nb, 3)
        return spec, nb, prm, (lo, up)
    spec = SPECS[name](); nb = 4
    return spec, nb, None, (cf.quadrotor_bounds(nb) if name == "D8" else cf.manipulator_bounds(nb, narms=2))


@pytest.mark.parametrize("name", ["O", "OF", "D8", "E8"])
def test_rows_at_breakpoints_equal_eval(name):
    spec, nb, prm, (lo, up) = _case(name)
    p = api.Plan(spec, 0)
    if prm is not None:
        p.set_params(dev(prm))
    x = np.random.default_rng(4).normal(size=(nb, spec.nC))
    c = p.eval(dev(x), 0)["c"].cpu().numpy()
    cn = c[:, spec.nnlic:spec.nnlic + spec.nnltc * spec.nbps].reshape(nb, spec.nnltc, spec.nbps)
    out = p.check(dev(x), dev(lo), dev(up), dev(spec.bps), want_rows=True)
    torch.cuda.synchronize()
    rows = out["rows"].cpu().numpy()
    print(f"{name}: rows vs eval {rel(rows, cn):.2e}")
    assert rows.shape == cn.shape and rel(rows, cn) <= TOL
    compare(spec, out, cn, lo, up, name)   # eval's rows as the reference of the violations


# ---- 2. dense times against the fine-spec oracle ----
@pytest.fixture(scope="module")
def oplan():
    return api.Plan(cf.config_O(ninterv=4), 0)


@pytest.mark.parametrize("ntimes,shuffle", [(1, False), (63, False), (64, False), (65, True), (81, False), (257, False)])
def test_dense_times_match_oracle(oplan, ntimes, shuffle):
    spec, nb = oplan.spec, 8
    rng = np.random.default_rng(ntimes)
    times = np.array([1.7]) if ntimes == 1 else tgrid(spec, ntimes)
    if shuffle:
        times = rng.permutation(times)   # nothing may assume order
    x = rng.normal(size=(nb, spec.nC))
    ref = ref_rows(spec, x, times)
    lo, up = rand_bounds(spec, nb, ref)
    out = oplan.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)
    torch.cuda.synchronize()
    vref = compare(spec, out, ref, lo, up, f"O dense {ntimes}")
    assert (vref.reshape(nb, -1).max(axis=1) > 0).any()


# ---- 3. the motivating case ----
def test_obstacle_solutions_cut_the_obstacle_between_breakpoints(oplan):
    spec, nb = oplan.spec, 8
    lo, up = cf.obstacle_bounds(nb)
    x = dev(np.ones((nb, spec.nC)))
    sol = oplan.solve(dev(lo), dev(up), x, api.default_opts(hessian=1))
    bp = np.asarray(spec.bps)
    times = np.append((bp[:-1, None] + (bp[1:] - bp[:-1])[:, None] * np.arange(4)[None, :] / 4.0).ravel(), bp[-1])   # 81 uniform times
    assert times.size == 81 and np.abs(np.diff(times) - 5.0 / 80).max() <= 1e-12
    out = oplan.check(x, dev(lo), dev(up), dev(times), want_rows=True)
    at_bps = oplan.check(x, dev(lo), dev(up), dev(times[::4]))
    torch.cuda.synchronize()
    assert (sol["inform"].cpu().numpy() == 0).all()
    assert (times[::4] == bp).all()
    vb = at_bps["viol"].cpu().numpy(); viol = out["viol"].cpu().numpy()
    print("viol at the breakpoints", vb, "\nviol at 81 times", viol)
    assert (vb <= 1e-6).all()
    ref = ref_rows(spec, x.cpu().numpy(), times)
    compare(spec, out, ref, lo, up, "O solved")
    vmax = violations(spec, ref, lo, up).reshape(nb, -1).max(axis=1)
    print("oracle at the same x", vmax, "relative difference", rel(viol, vmax))
    assert rel(viol, vmax) <= TOL
    assert (viol > 0.1).sum() >= nb // 2


# ---- 4. shared grid with two basis classes, a linear row and two nonlinear rows ----
@pytest.fixture(scope="module")
def tplan():
    return api.Plan(cf.config_T(), 0)


def test_two_classes_linear_and_nonlinear_rows(tplan):
    spec, nb = tplan.spec, 6
    assert spec.nltc == 1 and spec.nnltc == 2 and len(set(spec.order)) == 2
    rng = np.random.default_rng(8)
    times = tgrid(spec, 150)
    x = rng.normal(size=(nb, spec.nC))
    ref = ref_rows(spec, x, times)
    lo, up = rand_bounds(spec, nb, ref)
    out = tplan.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)
    torch.cuda.synchronize()
    vref = compare(spec, out, ref, lo, up, "T")
    assert {int(r) for r in out["where"].cpu().numpy()[:, 0]} - {-1}, "no violation in the whole batch"
    assert (vref[:, 0].max(axis=1) > 0).any() and (vref[:, 1:].max(axis=(1, 2)) > 0).any()   # rows of both kinds violate somewhere
    # an infinite bound on one side is absent, whatever its sign: with every bound infinite nothing is violated
    s = traj_slots(spec)
    lo2, up2 = lo.copy(), up.copy()
    lo2[:, s] = INF; up2[:, s] = -INF
    o2 = tplan.check(dev(x), dev(lo2), dev(up2), dev(times))
    assert (o2["viol"].cpu().numpy() == 0).all() and (o2["where"].cpu().numpy() == -1).all()
    lo3, up3 = lo.copy(), up.copy()
    lo3[:, s[0]] = -INF; up3[:, s[1]] = INF; lo3[:, s[2]] = INF   # one side each
    o3 = tplan.check(dev(x), dev(lo3), dev(up3), dev(times), want_rows=True)
    compare(spec, o3, ref, lo3, up3, "T one-sided")


@pytest.mark.parametrize("pair", [(1, 2), (0, 2), (0, 1)])
def test_equal_violations_report_the_lower_row(tplan, pair):
    """one time, two rows that violate by exactly the same amount: the bounds are built from the row values the device reports, with an
    offset for which c - (c - d) is the same double for both rows"""
    spec = tplan.spec
    rng = np.random.default_rng(12)
    x = rng.normal(size=(1, spec.nC))
    s = traj_slots(spec)
    lo = np.full((1, spec.nbounds), -INF); up = np.full((1, spec.nbounds), INF)
    found = False
    for tv in np.linspace(0.1, 1.9, 19):   # (inside the knot range [0, 2])
        times = np.array([tv])
        rows = tplan.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)["rows"].cpu().numpy()[0, :, 0]
        for d in (0.25, 0.5, 1.0, 2.0, 0.125):
            u = rows - d
            if rows[pair[0]] - u[pair[0]] == rows[pair[1]] - u[pair[1]]:
                found = True
                break
        if found:
            break
    assert found, "no offset gives an exact tie"
    up[0, s[pair[0]]] = u[pair[0]]; up[0, s[pair[1]]] = u[pair[1]]
    out = tplan.check(dev(x), dev(lo), dev(up), dev(times))
    assert out["viol"].cpu().numpy()[0] == rows[pair[0]] - u[pair[0]]
    assert tuple(out["where"].cpu().numpy()[0]) == (min(pair), 0)


# ---- 5. per-problem grids ----
def _debug_check(plan, x, lo, up, times, stride, cap):
    """ntg_debug_batch_check: ntg_batch_check with the scratch cap of the per-problem time tables stated (forces several chunks)"""
    L = api.lib()
    L.ntg_debug_batch_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    nb, nt = x.shape[0], times.shape[-1]
    viol = torch.zeros(nb, dtype=torch.float64, device=x.device); where = torch.zeros((nb, 2), dtype=torch.int32, device=x.device)
    rows = torch.zeros((nb, plan.spec.nltc + plan.spec.nnltc, nt), dtype=torch.float64, device=x.device)
    rc = L.ntg_debug_batch_check(plan.h, nb, x.data_ptr(), lo.data_ptr(), up.data_ptr(), nt, times.data_ptr(), stride,
                                 viol.data_ptr(), where.data_ptr(), rows.data_ptr(), None, cap)
    assert rc == 0, L.ntg_last_error().decode()
    torch.cuda.synchronize()
    return dict(viol=viol, where=where, rows=rows)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_per_problem_grids_and_chunks():
    spec, nb, ntimes = cf.config_O(ninterv=4), 8, 131
    knots, bps = grids_for(spec, nb, warp=0.2)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    rng = np.random.default_rng(6)
    x = rng.normal(size=(nb, spec.nC))
    u = np.linspace(0.0, 1.0, ntimes)
    times = np.minimum(knots[:, :1] + (knots[:, -1:] - knots[:, :1]) * u[None, :], knots[:, -1:])   # every problem over its own horizon
    shared = np.linspace(0.0, knots[:, -1].min(), ntimes)                                            # inside every problem's knot range
    ref_own = np.concatenate([ref_rows(spec_on(spec, knots[b], bps[b]), x[b:b + 1], times[b]) for b in range(nb)])
    ref_sh = np.concatenate([ref_rows(spec_on(spec, knots[b], bps[b]), x[b:b + 1], shared) for b in range(nb)])
    lo, up = rand_bounds(spec, nb, ref_own)
    xd, lod, upd = dev(x), dev(lo), dev(up)
    own = p.check(xd, lod, upd, dev(times), want_rows=True)
    sh = p.check(xd, lod, upd, dev(shared), want_rows=True)
    torch.cuda.synchronize()
    compare(spec, own, ref_own, lo, up, "grids, own times")
    compare(spec, sh, ref_sh, lo, up, "grids, shared times")
    assert np.abs(ref_own - ref_sh).max() > 1e-3
    # the batch in chunks of 1 and of 3 problems (3 + 3 + 2): bit for bit the one-chunk result
    per = ntimes * (spec.order[0] * spec.maxderiv[0] * 8 + 4)
    for cap in (1, 3 * per + 8):
        assert _same(_debug_check(p, xd, lod, upd, dev(times), ntimes, cap), own)
        assert _same(_debug_check(p, xd, lod, upd, dev(shared), 0, cap), sh)
    with pytest.raises(api.NtgError, match="-2"):   # the grids are for exactly this batch
        p.check(xd[:3], lod[:3], upd[:3], dev(shared))
    p.clear_grids()


# ---- 6. family modules ----
@pytest.fixture(scope="module")
def fams():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    ids = {m: api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", m + ".hip"))) for m in ("unicycle", "tracking")}
    ids["cb"] = fo.Callbacks(fo.build_shim("unicycle_host"), "uni_")
    return ids


def test_unicycle_module_rows_match_its_oracle(fams):
    spec, nb = cf.config_U(fams["unicycle"]), 8
    p = api.Plan(spec, 0)
    rng = np.random.default_rng(9)
    x = rng.normal(size=(nb, spec.nC))
    times = tgrid(spec, 140)
    ref = ref_rows(spec, x, times, cb=fams["cb"])
    lo, up = rand_bounds(spec, nb, ref)
    out = p.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)
    torch.cuda.synchronize()
    assert out["rows"].shape == (nb, 2, 140)
    compare(spec, out, ref, lo, up, "unicycle")


def test_tracking_module_is_refused(fams):
    spec, nb = cf.config_TR(fams["tracking"]), 4
    p = api.Plan(spec, 0)
    prm, lo, up = cf.tracking_problems(spec, nb)
    p.set_params(dev(prm))
    with pytest.raises(api.NtgError, match="-4"):   # NTG_E_UNSUPPORTED: its data exists at breakpoints only
        p.check(dev(np.ones((nb, spec.nC))), dev(lo), dev(up), dev(spec.bps))


# ---- 7. refusals, degenerate calls, determinism ----
def test_refusals_and_degenerate_calls(oplan):
    spec, nb = oplan.spec, 4
    lo, up = cf.obstacle_bounds(nb)
    x, lod, upd, t = dev(np.ones((nb, spec.nC))), dev(lo), dev(up), dev(tgrid(spec, 9))
    L, st = api.lib(), None
    raw = lambda plan, batch, nt, stride, v, w, r: L.ntg_batch_check(plan.h, batch, x.data_ptr(), lod.data_ptr(), upd.data_ptr(), nt,
                                                                       t.data_ptr(), stride, v, w, r, st)
    viol = torch.full((nb,), 7.0, dtype=torch.float64, device="cuda:0")
    assert raw(oplan, 0, 9, 0, viol.data_ptr(), None, None) == 0 and raw(oplan, nb, 0, 0, viol.data_ptr(), None, None) == 0
    assert (viol.cpu().numpy() == 7.0).all()                                   # nothing ran
    assert raw(oplan, nb, 9, 0, None, None, None) == -2                        # no output asked for
    assert raw(oplan, nb, 9, 5, viol.data_ptr(), None, None) == -2             # times_stride < ntimes
    assert raw(oplan, nb, 9, 9, viol.data_ptr(), None, None) == -2             # per-problem times without per-problem grids
    assert "per-problem grids" in L.ntg_last_error().decode()
    with pytest.raises(api.NtgError):
        oplan.check(x, lod, upd, dev(np.zeros((nb, 9))))
    kin = api.Plan(cf.config_B(), 0)                                           # no trajectory rows
    klo, kup = cf.kincar_random_bounds(1, nb)
    with pytest.raises(api.NtgError, match="no trajectory rows to check"):
        kin.check(dev(np.ones((nb, kin.spec.nC))), dev(klo), dev(kup), t)
    of = api.Plan(cf.config_OF(3, ninterv=4), 0)                               # parameters: not set, then set for another batch
    prm, flo, fup = cf.obstacle_field_problems(nb, 3)
    xf = dev(np.ones((nb, of.spec.nC)))
    with pytest.raises(api.NtgError, match="-2"):
        of.check(xf, dev(flo), dev(fup), t)
    of.set_params(dev(prm))
    assert of.check(xf, dev(flo), dev(fup), t)["viol"].shape == (nb,)
    with pytest.raises(api.NtgError, match="-2"):
        of.check(xf[:2], dev(flo[:2]), dev(fup[:2]), t)
    # rows only: no bounds needed
    rows = torch.zeros((nb, 1, 9), dtype=torch.float64, device="cuda:0")
    assert L.ntg_batch_check(oplan.h, nb, x.data_ptr(), None, None, 9, t.data_ptr(), 0, None, None, rows.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows, oplan.check(x, lod, upd, t, want_rows=True)["rows"])


def test_no_violation_gives_minus_one_and_results_do_not_depend_on_the_batch(oplan):
    spec, nb = oplan.spec, 8
    rng = np.random.default_rng(21)
    x = rng.normal(size=(nb, spec.nC))
    times = tgrid(spec, 300)
    ref = ref_rows(spec, x, times)
    lo, up = cf.obstacle_bounds(nb)
    lo[:4, -1] = ref[:4].min() - 1.0   # the first four problems cannot violate,
    lo[4:, -1] = np.median(ref[4:, 0], axis=1)   # the others do at half of their times
    xd, lod, upd, td = dev(x), dev(lo), dev(up), dev(times)
    a = oplan.check(xd, lod, upd, td, want_rows=True)
    b = oplan.check(xd, lod, upd, td, want_rows=True)
    torch.cuda.synchronize()
    assert _same(a, b)                                                        # call to call
    viol, where = a["viol"].cpu().numpy(), a["where"].cpu().numpy()
    assert (viol[:4] == 0).all() and (where[:4] == -1).all() and (viol[4:] > 0).all() and (where[4:] >= 0).all()
    compare(spec, a, ref, lo, up, "O mixed")
    sub = oplan.check(xd[2:7].contiguous(), lod[2:7].contiguous(), upd[2:7].contiguous(), td, want_rows=True)
    assert all(torch.equal(sub[k], a[k][2:7]) for k in a)                     # a subset of the batch
    perm = torch.tensor(rng.permutation(nb), device="cuda:0")
    pr = oplan.check(xd[perm].contiguous(), lod[perm].contiguous(), upd[perm].contiguous(), td, want_rows=True)
    assert all(torch.equal(pr[k], a[k][perm]) for k in a)                     # a permuted batch


def test_host_callback_plans_are_refused():
    """a plan of host function pointers has no device row functions: NTG_E_UNSUPPORTED, before anything is launched"""
    spec = dataclasses.replace(cf.config_O(ninterv=4), family=-1)   # NTG_FAM_HOST
    p = api.Plan(spec, 0)
    nb = 2
    lo, up = cf.obstacle_bounds(nb)
    with pytest.raises(api.NtgError, match="-4") as e:
        p.check(dev(np.ones((nb, spec.nC))), dev(lo), dev(up), dev(tgrid(spec, 9)))
    assert "host-callback plans" in str(e.value)


# ---- the instances of the families without nonlinear rows (linear trajectory rows only), by flag size ----
def _with_ltc(spec, nrows, seed):
    ltc = np.round(np.random.default_rng(seed).uniform(-1, 1, (nrows, spec.nz)), 3)
    nl = spec.nlic + nrows + spec.nlfc
    return dataclasses.replace(spec, ltc=ltc, lin_ineq=[0] * spec.nlic + [1] * nrows + [0] * spec.nlfc if nl else ())


@pytest.mark.parametrize("name", ["A", "B", "M", "K8"])
def test_linear_rows_of_kincar_and_vanderpol(name):
    """vanderpol (flag of 3) and kincar with 2, 6 and 8 outputs (flags of 6, 18 and 24: the 6-, 18- and 64-entry instances)"""
    base = {"A": cf.config_A, "B": cf.config_B, "M": cf.config_M,
            "K8": lambda: cf._kincar_spec(4, 6, 3, 20, 101, 5.0, "K8:kincar-8out-k6-l20")}[name]()
    spec, nb = _with_ltc(base, 2, 31), 4
    p = api.Plan(spec, 0)
    rng = np.random.default_rng(32)
    x = rng.normal(size=(nb, spec.nC))
    times = tgrid(spec, 200)
    ref = ref_rows(spec, x, times)
    lo, up = rand_bounds(spec, nb, ref)
    out = p.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)
    torch.cuda.synchronize()
    assert out["rows"].shape == (nb, 2, 200)
    vref = compare(spec, out, ref, lo, up, name + " linear rows")
    assert (vref.reshape(nb, -1).max(axis=1) > 0).any()


def test_equal_violations_at_different_times_report_the_first(oplan):
    """the time of every problem's largest violation repeated at indices of other lanes, the other wave and other tiles: all copies
    violate by the same double, the smallest time index must be reported (the wave, workgroup and tile steps of the reduction)"""
    spec, nb = oplan.spec, 4
    rng = np.random.default_rng(41)
    x = rng.normal(size=(nb, spec.nC))
    base = tgrid(spec, 300)
    lo, up = cf.obstacle_bounds(nb)
    rows = oplan.check(dev(x), dev(lo), dev(up), dev(base), want_rows=True)["rows"].cpu().numpy()[:, 0]
    lo[:, -1] = rows.max(axis=1) + 1.0                      # lower bound above every value: the largest violation is at the row's minimum
    for b in range(nb):
        j = int(np.argmin(rows[b]))
        times = base.copy()
        times[[299, 205, 130, 100, 37]] = base[j]            # tiles 2, 1, 1, 0 (second wave), 0 (first wave)
        out = oplan.check(dev(x), dev(lo), dev(up), dev(times), want_rows=True)
        r = out["rows"].cpu().numpy()[b, 0]
        v = lo[b, -1] - r
        first = int(np.argmax(v))                            # numpy's argmax is the first of equal maxima
        assert (v == v.max()).sum() >= 5 and first == min(j, 37)
        assert out["viol"].cpu().numpy()[b] == v.max()
        assert tuple(out["where"].cpu().numpy()[b]) == (0, first)
