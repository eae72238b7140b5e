"""-m gpu: user problem families loaded from modules (ntg_family_load) through every batched entry point.

  unicycle        (ntg_amd/modules/unicycle.hip, all six callback slots) against the CPU oracle fed by a host shim compiled from the
                  same family header (tests/modules/unicycle_host.cpp, tests/family_oracle.py)
  testfam_module  (the built-in NTG_FAM_TESTFAM restated as a module) bit for bit against the built-in family on a plan where the
                  built-in runs its generic instance

Tolerances: evaluation 1e-12 relative; optimum |dF| <= 1e-9 max(1, |F|), |dx| <= 1e-6 max(1, |x|inf) where both implementations end at
inform 0, for at least half of those; the end game of the augmented-Lagrangian loop on an active nonlinear row is decided at rounding
level, so as in tests/test_gpu_constrained.py the batch as a whole is held to 1e-6 / 1e-4."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import orc
import family_oracle as fo
from ntg_amd import api, configs as cf
from gpu_common import dev, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fams():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    ids = {m: api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", m + ".hip"))) for m in ("unicycle", "testfam_module")}
    ids["cb"] = fo.Callbacks(fo.build_shim("unicycle_host"), "uni_")
    return ids


@pytest.fixture(scope="module")
def uplan(fams):
    return api.Plan(cf.config_U(fams["unicycle"]), 0)


def _oracle_solve(spec, cb, lo, up, x0, hessian, **kw):
    return fo.solve_batch(spec, cb, lo, up, x0, orc.default_opts(hessian=hessian, **kw))


def _close(xg, og, ref, b, tf=1e-9, tx=1e-6):
    return abs(og[b] - ref["objective"][b]) <= tf * max(1.0, abs(ref["objective"][b])) and \
        np.abs(xg[b] - ref["x"][b]).max() <= tx * max(1.0, np.abs(ref["x"][b]).max())


def test_unicycle_eval_matches_oracle(fams, uplan):
    spec = uplan.spec
    nb = 16
    x = np.random.default_rng(11).normal(size=(nb, spec.nC))
    ev = uplan.eval(dev(x), 2, want_dense_jac=True)
    torch.cuda.synchronize()
    f, g, c = ev["f"].cpu().numpy(), ev["g"].cpu().numpy(), ev["c"].cpu().numpy()
    J, jb = ev["cJac"].cpu().numpy(), ev["jband"].cpu().numpy()
    off = uplan.tables()["off"]
    P, koff, iC = spec.nbps, np.cumsum([0] + spec.order[:-1]), np.cumsum([0] + spec.ncoef[:-1])
    rbp = [0] * spec.nnlic + [i for _ in range(spec.nnltc) for i in range(P)] + [P - 1] * spec.nnlfc
    zero = np.zeros(spec.nbounds)
    for b in range(nb):
        pr = fo.Problem(spec, fams["cb"], zero, zero)
        ref = pr.eval(x[b])
        pr.close()
        assert abs(f[b] - ref["f"]) <= 1e-12 * max(1.0, abs(ref["f"]))
        assert rel(g[b], ref["g"]) <= 1e-12 and rel(c[b], ref["c"]) <= 1e-12 and rel(J[b], ref["cJac"]) <= 1e-12
        # banded Jacobian: row r holds, per output, the k entries starting at the block offset of its breakpoint
        Jb = np.zeros_like(ref["cJac"])
        for r in range(spec.ncnln):
            for o in range(spec.nout):
                k = spec.order[o]
                Jb[r, iC[o] + off[o, rbp[r]]:iC[o] + off[o, rbp[r]] + k] = jb[b, r, koff[o]:koff[o] + k]
        assert rel(Jb, ref["cJac"]) <= 1e-12


@pytest.mark.parametrize("hessian", [0, 1])
def test_unicycle_solves_match_oracle(fams, uplan, hessian):
    spec = uplan.spec
    nb, P = 256, spec.nbps
    lo, up = cf.unicycle_bounds(nb)
    x = dev(np.ones((nb, spec.nC)))
    out = uplan.solve(dev(lo), dev(up), x, api.default_opts(hessian=hessian))
    torch.cuda.synchronize()
    xg, og, inf = x.cpu().numpy(), out["objective"].cpu().numpy(), out["inform"].cpu().numpy()
    ref = _oracle_solve(spec, fams["cb"], lo, up, np.ones((nb, spec.nC)), hessian)
    # both run the same augmented-Lagrangian SQP, but its end game on an active nonlinear row is decided at rounding level: as in
    # tests/test_gpu_constrained.py accept NPSOL's "optimal" (0) and "optimal, not to requested accuracy" (1), and require the clear
    # majority of the batch at the oracle's point
    assert np.isin(inf, (0, 1)).all() and np.isin(ref["inform"], (0, 1)).all()
    assert (inf == 0).mean() >= 0.85 and (ref["inform"] == 0).mean() >= 0.9
    same = np.array([_close(xg, og, ref, b, 1e-6, 1e-4) for b in range(nb)])
    assert same.mean() >= 0.9, same.mean()
    # (to BASELINE's acceptance tolerances: about 0.4 of the batch with the identity cold start, 0.8 with the preconditioner)
    tight = np.array([_close(xg, og, ref, b) for b in range(nb)])
    assert tight.mean() >= 0.3, tight.mean()
    # the constraint path is exercised: the lateral-acceleration band is active at the optimum of a visible share of the batch
    c = uplan.eval(x, 0)["c"].cpu().numpy()
    cross = np.abs(c[:, 1 + P:1 + 2 * P]).max(axis=1)
    active = (up[:, 7] - cross) <= 1e-5 * up[:, 7]
    assert active.mean() >= 0.05, active.mean()


def test_unicycle_fixed_majors(fams):
    """50 fixed majors (the fixed-work mode takes plans without nonlinear rows: the unicycle's cost slots and linear rows only)"""
    spec = dataclasses.replace(cf.config_U(fams["unicycle"]), nnlic=0, nnltc=0, nnlfc=0, icav=(), tcav=(), fcav=())
    p = api.Plan(spec, 0)
    nb = 64
    lo, up = cf.unicycle_bounds(nb)
    lo, up = lo[:, :5].copy(), up[:, :5].copy()
    x = dev(np.ones((nb, spec.nC)))
    out = p.solve(dev(lo), dev(up), x, api.default_opts(itlim=50, fixed_iters=1))
    torch.cuda.synchronize()
    ref = _oracle_solve(spec, fams["cb"], lo, up, np.ones((nb, spec.nC)), 0, itlim=50, fixed_iters=1)
    # a problem that reaches the optimum to rounding level before the 50th major stops there (inform 0), in both implementations; which
    # major that is (47 to 50 here) is decided by rounding noise, so the evaluation counts are not compared problem by problem
    it = out["iters"].cpu().numpy()
    assert (it <= 50).all() and (it >= 45).all() and np.isin(out["inform"].cpu().numpy(), (0, 4)).all(), it
    og = out["objective"].cpu().numpy()
    assert (np.abs(og - ref["objective"]) <= 1e-7 * np.maximum(1.0, np.abs(ref["objective"]))).all()


def _testfam_case(nb=6):
    """config_T with two outputs (the built-in family's generic instance) and feasible bounds on every row (as test_gpu_constrained)"""
    spec = cf.config_T(nout=2); spec.ltc = np.zeros((0, spec.nz))
    rng = np.random.default_rng(5)
    blin = (rng.normal(size=(nb, spec.nC)) * 0.3) @ orc.export_tables(spec)["A"].T
    lo = np.zeros((nb, spec.nbounds)); up = np.zeros((nb, spec.nbounds))
    lo[:, 0:4] = up[:, 0:4] = blin
    lo[:, 4], up[:, 4] = 0.2, 3.0
    lo[:, 5], up[:, 5] = -1e20, 40.0
    lo[:, 6], up[:, 6] = -6.0, 6.0
    lo[:, 7] = up[:, 7] = 0.5
    return spec, lo, up


def _run(p, lo, up, x0, opts):
    x = dev(x0)
    out = p.solve(dev(lo), dev(up), x, opts)
    torch.cuda.synchronize()
    return {"x": x.cpu().numpy(), **{k: v.cpu().numpy() for k, v in out.items()}}


def _ev(p, x0):
    ev = p.eval(dev(x0), 2)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in ev.items()}


def _bitwise(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_testfam_module_is_the_builtin_bit_for_bit(fams):
    spec, lo, up = _testfam_case()
    specm = dataclasses.replace(spec, family=fams["testfam_module"])
    pb, pm = api.Plan(spec, 0), api.Plan(specm, 0)
    x0 = np.random.default_rng(3).normal(size=(lo.shape[0], spec.nC))
    assert _bitwise(_ev(pb, x0), _ev(pm, x0))
    for hessian in (0, 1):
        o = api.default_opts(hessian=hessian, itlim=3000)
        assert pb.solve_kernel(6, o) == pm.solve_kernel(6, o) == "sqp_kernel"
        rb, rm = _run(pb, lo, up, np.ones_like(x0), o), _run(pm, lo, up, np.ones_like(x0), o)
        assert _bitwise(rb, rm), hessian


def test_two_modules_and_builtins_interleaved(fams, uplan):
    """each family gives in an interleaved sequence exactly what it gives alone (the modules' same-named kernels stay apart)"""
    spec, lo, up = _testfam_case()
    pb, pm = api.Plan(spec, 0), api.Plan(dataclasses.replace(spec, family=fams["testfam_module"]), 0)
    pk = api.Plan(cf.config_B(), 0)
    nbu = 32
    ulo, uup = cf.unicycle_bounds(nbu, seed=9)
    klo, kup = cf.kincar_random_bounds(1, 8)
    o = api.default_opts(hessian=1, itlim=3000)
    runs = {"uni": lambda: _run(uplan, ulo, uup, np.ones((nbu, uplan.spec.nC)), o),
            "mod": lambda: _run(pm, lo, up, np.ones((6, spec.nC)), o),
            "tf": lambda: _run(pb, lo, up, np.ones((6, spec.nC)), o),
            "kin": lambda: _run(pk, klo, kup, np.ones((8, pk.spec.nC)), o)}
    alone = {k: f() for k, f in runs.items()}
    for k in ("mod", "uni", "kin", "tf", "uni", "mod"):
        assert _bitwise(runs[k](), alone[k]), k


def test_hessian_2_on_a_module_plan_is_hessian_1(fams, uplan):
    nb = 32
    lo, up = cf.unicycle_bounds(nb, seed=4)
    o1, o2 = api.default_opts(hessian=1), api.default_opts(hessian=2)
    assert uplan.solve_kernel(nb, o2) == "sqp_kernel"
    x0 = np.ones((nb, uplan.spec.nC))
    assert _bitwise(_run(uplan, lo, up, x0, o1), _run(uplan, lo, up, x0, o2))


def test_unicycle_per_problem_grids_vs_oracle(fams):
    from test_gpu_grids import grids_for, spec_on
    spec = cf.config_U(fams["unicycle"])
    p = api.Plan(spec, 0)
    nb = 16
    knots, bps = grids_for(spec, nb, seed=6)
    lo, up = cf.unicycle_bounds(nb, seed=6)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    x = dev(np.ones((nb, spec.nC)))
    out = p.solve(dev(lo), dev(up), x, api.default_opts(hessian=0))
    torch.cuda.synchronize()
    xg, og, inf = x.cpu().numpy(), out["objective"].cpu().numpy(), out["inform"].cpu().numpy()
    nsame = 0
    for b in range(nb):
        ref = _oracle_solve(spec_on(spec, knots[b], bps[b]), fams["cb"], lo[b:b + 1], up[b:b + 1], np.ones((1, spec.nC)), 0)
        nsame += abs(og[b] - ref["objective"][0]) <= 1e-7 * max(1.0, abs(ref["objective"][0])) and \
            np.abs(xg[b] - ref["x"][0]).max() <= 1e-5 * max(1.0, np.abs(ref["x"][0]).max())
    assert nsame >= 3 * nb // 4, nsame   # identity cold start: the same share as on the shared grid (~0.93 of 256)


def test_unicycle_mpc_run_is_the_host_loop(fams, uplan):
    spec = uplan.spec
    nb, nsteps, sbp, sknot = 32, 4, 5, 1
    lo, up = cf.unicycle_bounds(nb, seed=8)
    cold, warm = api.default_opts(hessian=1), api.default_opts(hessian=1, warm_start=1)
    nbytes = uplan.workspace_bytes(nb, warm)
    work1 = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    x1, lo1, up1 = dev(np.ones((nb, spec.nC))), dev(lo), dev(up)
    for step in range(nsteps):
        uplan.solve(lo1, up1, x1, warm if step > 0 else cold, work=work1)
        uplan.mpc_shift(x1, lo1, up1, sbp, sknot)
        uplan.mpc_shift_multipliers(nb, sbp, warm, work1)
    work2 = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    x2, lo2, up2 = dev(np.ones((nb, spec.nC))), dev(lo), dev(up)
    uplan.mpc_run(x2, lo2, up2, nsteps, sbp, sknot, warm, work=work2)
    torch.cuda.synchronize()
    assert torch.equal(x1, x2) and torch.equal(lo1, lo2) and torch.equal(up1, up2)


def test_plan_creation_refusals(fams):
    spec = cf.config_U(fams["unicycle"])
    bad_d = dataclasses.replace(spec, maxderiv=[4, 4], lic=np.zeros((3, 8)), lfc=np.zeros((2, 8)))
    with pytest.raises(api.NtgError, match="error -4"):
        api.Plan(bad_d, 0)
    with pytest.raises(api.NtgError, match="error -2"):
        api.Plan(dataclasses.replace(spec, nnltc=3), 0)
    with pytest.raises(api.NtgError, match="error -2"):
        api.Plan(dataclasses.replace(spec, family=127), 0)
