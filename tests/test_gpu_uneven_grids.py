"""-m gpu: shared grids with uneven knots and an uneven number of breakpoints per knot interval (tests/uneven_grids.py) against the oracle,
run live on the same spec, through the C ABI.

Every other plan of the suite has uniform knots and 5, 5, ..., 6 breakpoints per interval.  Here the intervals differ in length by a factor
of 1.9 and hold 0 .. 7 breakpoints, the first of each on a knot and one of them an ulp below a knot: the breakpoint groups of the plan
(NtgDims::ig_n / igb), the per-interval tables of eval_interval_kernel and sqp_wave_kernel (6 slots per interval, node weights, interval
lengths), the column widths of the column form, the group colours of the Newton / QP tables and the singular branch of the
preconditioner all see something other than the one pattern they have been run with.  The oracle is pinned on these grids first, on the
CPU: tests/test_oracle_pgs.py (scipy), tests/test_oracle_vs_reference.py (ref_U20 / U16 / UO / UD8: the reference's own code, bit for
bit), tests/test_uneven_grids_oracle.py (the conditions the solves below rely on).

Tolerances are the project's own:
  tables 1e-13, offsets exact; f, g, c, Jacobian 1e-12 relative, band positions identical           (tests/test_gpu_basis_eval.py)
  optimum |dF| <= 1e-9 max(1, |F|), |dx| <= 1e-6 max(1, |x|inf), |A x - b| <= 1e-8                  (tests/test_gpu_solve.py)
  fixed work: gpu_common.same_work, objective 1e-7, x 1e-5                                          (tests/test_gpu_solve.py)
  Newton and QP modes: majors within 3, objective 1e-9, x 1e-6                                      (tests/test_gpu_newton.py)

Kernels (Plan.solve_kernel): kincar on C20 (2, 4, 6 outputs) and on C16 with 4 outputs is solved by sqp_wave_kernel; C16 with 2 or 6 outputs
by sqp_kernel, because ntg_wave_plan (fam_kincar_wave.hip) takes 16 knot intervals for four outputs only -- the only 16-interval
instances that are compiled (`D.nout == 4 && wave_match(..., 16)`); C20_7 (ig_n = 0: a group of 7) and C20_0 (19 groups on 20 intervals:
ig_n = 19, ncoef != 3 ig_n + 3) by sqp_kernel; every plan with nonlinear rows by sqp_kernel.
The library refuses none of these grids."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import orc
from ntg_amd import api, configs as cf
from gpu_common import plan_for, dev, rel, same_work
from test_gpu_large import _band_from_dense
import uneven_grids as ug

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE_PLAN = {"U20": "K3-C20", "U16": "K2-C16", "UO": "O-C20", "UD8": "D8-C8"}
_plans = {}
_orc = {}


def plan(name):
    """the plan of ug.ALL[name], built once (the two kincar fixtures' plans are gpu_common's U20 / U16)"""
    shared = {"K3-C20": "U20", "K2-C16": "U16"}
    if name in shared:
        return plan_for(shared[name])
    if name not in _plans:
        _plans[name] = api.Plan(ug.ALL[name](), 0)
    return _plans[name]


def gold(name):
    return dict(np.load(os.path.join(GOLD, f"ref_{name}.npz")))


def gpu_solve(p, lo, up, want_lambda=False, **kw):
    x = torch.ones((lo.shape[0], p.spec.nC), dtype=torch.float64, device="cuda:0")
    out = p.solve(dev(lo), dev(up), x, api.default_opts(**kw), want_lambda=want_lambda)
    torch.cuda.synchronize()
    return x.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


def orc_solve(name, lo, up, **kw):
    """the oracle's solve of the same batch from x0 = 1, computed once per (spec, batch, options)"""
    key = (name, lo.shape[0], tuple(sorted(kw.items())))
    if key not in _orc:
        spec = plan(name).spec
        _orc[key] = orc.solve_batch(spec, lo, up, np.ones((lo.shape[0], spec.nC)), orc.default_opts(**kw), nthreads=8)
    return _orc[key]


def check_optimum(p, x, out, ref, lo, compare_x=True, obj_tol=None, feas_tol=1e-8):
    """inform 0, objective, x and feasibility of the linear rows (against the ORACLE's A), problem by problem; obj_tol [batch]: absolute
    tolerances of the objective in the place of 1e-9 max(1, |F|)"""
    A = orc.export_tables(p.spec)["A"]
    gap = np.abs(out["objective"] - ref["objective"]) / np.maximum(1.0, np.abs(ref["objective"]))
    feas = np.abs(x @ A.T - lo[:, :p.spec.nclin]).max(axis=1)
    print(f"  objective gap / max(1, |F|) {gap}  |A x - b| {feas}  majors {out['iters']} oracle {ref['iters']}")
    assert (out["inform"] == 0).all(), out["inform"]
    assert (ref["inform"] == 0).all(), ref["inform"]
    for b in range(x.shape[0]):
        tol = 1e-9 * max(1.0, abs(ref["objective"][b])) if obj_tol is None else obj_tol[b]
        assert abs(out["objective"][b] - ref["objective"][b]) <= tol, (b, out["objective"][b], ref["objective"][b], tol)
        if compare_x:
            assert np.abs(x[b] - ref["x"][b]).max() <= 1e-6 * max(1.0, np.abs(ref["x"][b]).max()), (b, np.abs(x[b] - ref["x"][b]).max())
        assert feas[b] <= feas_tol, (b, feas[b], feas_tol)


# -- a. tables and bounds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ug.ALL))
def test_tables(name):
    p = plan(name); spec = p.spec
    ref = orc.export_tables(spec); t = p.tables()
    assert np.array_equal(t["off"], ref["off"])                   # index work: exact (the breakpoint an ulp below a knot included)
    assert rel(t["blk"], ref["blk"]) <= 1e-13
    assert t["A"].shape == ref["A"].shape
    assert np.array_equal(t["A"] != 0, ref["A"] != 0)
    assert rel(t["A"], ref["A"]) <= 1e-13


@pytest.mark.parametrize("fx", list(FIXTURE_PLAN))
def test_bounds_expansion(fx):
    g = gold(fx)
    bl, bu = plan(FIXTURE_PLAN[fx]).bounds(dev(g["lowerb"][:1]), dev(g["upperb"][:1]))
    assert np.array_equal(bl.cpu().numpy()[0], g["bl"]) and np.array_equal(bu.cpu().numpy()[0], g["bu"])


# -- b. evaluation, kincar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", ug.KINCAR_LISTS)
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_eval_kincar_vs_oracle(ncars, counts):
    """37 problems (ragged problem slots in a wave for 2 and 4 outputs), the three NPSOL modes.  C20 and C20_thin (1 and 2 breakpoints in
    an interval) take eval_interval_kernel with 2, 4 and 6 outputs; C16 takes it with 6 outputs only: eval_interval_match declines 16
    intervals with 2 or 4 outputs, whose (64 / LP) nC = 408 staged doubles exceed the kernel's 6 x 64 slots, so the <2, ..., 16> and
    <4, ..., 16> instances of fam_kincar_chm.hip are never launched and these shapes take the breakpoint-lane kernels, like C20_7 and C20_0
    (seen with a library whose interval tables were spoiled on purpose: exactly the cases named here as the interval kernel's failed)."""
    p = plan(f"K{ncars}-{counts}"); spec = p.spec
    x = np.random.default_rng(11).normal(size=(37, spec.nC)) * 3.0
    ref = orc.eval_batch(spec, x, 2)
    for mode in (0, 1, 2):
        out = p.eval(dev(x), mode)
        if mode != 1:
            assert rel(out["f"].cpu().numpy(), ref["f"]) <= 1e-12, (mode, rel(out["f"].cpu().numpy(), ref["f"]))
        if mode != 0:
            assert rel(out["g"].cpu().numpy(), ref["g"]) <= 1e-12, (mode, rel(out["g"].cpu().numpy(), ref["g"]))


@pytest.mark.parametrize("fx", list(FIXTURE_PLAN))
def test_eval_matches_reference_fixture(fx):
    """the reference's own C code on these grids (tests/golden/make_golden.py)"""
    p = plan(FIXTURE_PLAN[fx]); spec = p.spec; g = gold(fx)
    out = p.eval(dev(g["x"]), 2, want_dense_jac=True)
    assert rel(out["f"].cpu().numpy(), g["f"]) <= 1e-12
    assert rel(out["g"].cpu().numpy(), g["g"]) <= 1e-12
    if spec.ncnln:
        assert rel(out["c"].cpu().numpy(), g["c"]) <= 1e-12
        J = out["cJac"].cpu().numpy()
        assert np.array_equal(J != 0, g["cJac"] != 0)
        assert rel(J, g["cJac"]) <= 1e-12


# -- c. evaluation, second trip of the persistent loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", [("K3-C20", 5000), ("M", 5000), ("K1-C20", 12325), ("B", 12325)])
def test_eval_second_trip_of_the_persistent_loop(name, batch):
    """eval_interval_kernel is persistent: its grid holds (launch_eval_interval) CUs x 4 workgroups x 4 waves x PW problems per wave, and a wave
    that has more to do takes a second trip of its loop with the coefficients prefetched during the first.  On the 256 CUs of an MI355X that
    is 4096 six-output problems (PW = 1) and 12288 two-output problems (PW = 3); the batches here, 5000 and 12325, are a little more
    than that, so that some waves take a second trip, the last of them with a ragged group of problems.  (On a part with fewer CUs every
    wave takes several trips; with more, raise the batches.)  Uniform grids (M, B) and the uneven C20."""
    p = plan(name) if name in ug.ALL else plan_for(name)
    spec = p.spec
    x = np.random.default_rng(13).normal(size=(batch, spec.nC)) * 3.0
    ref = orc.eval_batch(spec, x, 2, nthreads=8)
    out = p.eval(dev(x), 2)
    f = out["f"].cpu().numpy(); g = out["g"].cpu().numpy()
    assert rel(f, ref["f"]) <= 1e-12 and rel(g, ref["g"]) <= 1e-12
    # and problem by problem over the second trip (a stale or shifted problem there is a relative error of order 1, not 1e-12 of the batch's largest)
    first = 4096 if spec.nout == 6 else 12288
    assert (np.abs(f[first:] - ref["f"][first:]) <= 1e-12 * np.abs(ref["f"][first:])).all()
    assert (np.abs(g[first:] - ref["g"][first:]).max(axis=1) <= 1e-12 * np.abs(ref["g"][first:]).max(axis=1)).all()


# -- d. evaluation with nonlinear rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ug.SECOND_ORDER)
def test_eval_with_nonlinear_rows(name):
    p = plan(name); spec = p.spec
    x = np.random.default_rng(12).normal(size=(3, spec.nC)) * 0.5 + 1.0
    ev = p.eval(dev(x), 2, want_dense_jac=True)
    ref = orc.eval_batch(spec, x, 2, nthreads=3)
    assert rel(ev["f"].cpu().numpy(), ref["f"]) <= 1e-12
    assert rel(ev["g"].cpu().numpy(), ref["g"]) <= 1e-12
    assert rel(ev["c"].cpu().numpy(), ref["c"]) <= 1e-12
    J = ev["cJac"].cpu().numpy()
    assert np.array_equal(J != 0, ref["cJac"] != 0)
    assert rel(J, ref["cJac"]) <= 1e-12
    off = orc.export_tables(spec)["off"]
    jb = ev["jband"].cpu().numpy().reshape(3, spec.ncnln, -1)
    want = _band_from_dense(spec, ref["cJac"], off)
    assert np.isclose(np.abs(want).sum(), np.abs(ref["cJac"]).sum(), rtol=1e-12)   # nothing of the dense Jacobian lies outside the band
    assert jb.shape == want.shape and rel(jb, want) <= 1e-12
    assert np.array_equal(jb, _band_from_dense(spec, J, off))                      # the band carries the dense Jacobian's own numbers
    ev2 = p.eval(dev(x), 2)                                                        # the BANDONLY instance: bit-identical
    for key in ("f", "g", "c", "jband"):
        assert torch.equal(ev2[key], ev[key]), key


# -- e. solve to convergence, kincar -----------------------------------------------------------------------------------------------------
def wave_expected(ncars, counts):
    """see the module docstring: 16 knot intervals have wave instances for four outputs only"""
    return counts == "C20" or (counts == "C16" and ncars == 2)


@pytest.mark.parametrize("hessian", [0, 1])
@pytest.mark.parametrize("counts", ["C20", "C16"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_solve_to_convergence(ncars, counts, hessian):
    name = f"K{ncars}-{counts}"
    p = plan(name)
    lo, up = cf.kincar_random_bounds(ncars, ug.NB_CONV)
    kern = p.solve_kernel(ug.NB_CONV, api.default_opts(hessian=hessian))
    print(f"{name} hessian {hessian}: {kern}")
    assert kern == ("sqp_wave_kernel" if wave_expected(ncars, counts) else "sqp_kernel")
    x, out = gpu_solve(p, lo, up, hessian=hessian)
    ref = orc_solve(name, lo, up, hessian=hessian)
    check_optimum(p, x, out, ref, lo)
    if hessian == 1:
        assert out["iters"].max() <= 5
        assert np.abs(out["iters"] - ref["iters"]).max() <= 1, (out["iters"], ref["iters"])


# -- f. fixed majors ---------------------------------------------------------------------------------------------------------------------
def fixed_majors(ncars, counts, itlim):
    """itlim forced majors from the identity cold start (the benchmark mode), 16 problems: kernel, counts of majors and evaluations;
    returns the relative gaps of objective and x to the oracle"""
    name = f"K{ncars}-{counts}"
    p = plan(name)
    lo, up = cf.kincar_random_bounds(ncars, ug.NB_FIXED)
    kw = dict(itlim=itlim, fixed_iters=1)
    kern = p.solve_kernel(ug.NB_FIXED, api.default_opts(**kw))
    assert kern == ("sqp_wave_kernel" if wave_expected(ncars, counts) else "sqp_kernel")
    x, out = gpu_solve(p, lo, up, **kw)
    ref = orc_solve(name, lo, up, **kw)
    dobj, dx = rel(out["objective"], ref["objective"]), np.abs(x - ref["x"]).max() / np.abs(ref["x"]).max()
    print(f"{name} fixed {itlim}: {kern}  objective gap {dobj:.2e}  x gap {dx:.2e}  nfev {np.unique(out['nfev'])} oracle {np.unique(ref['nfev'])}")
    assert (out["iters"] == itlim).all() and (out["inform"] == 4).all()
    assert same_work(out["nfev"], ref["nfev"]), (out["nfev"], ref["nfev"])
    return dobj, dx


@pytest.mark.parametrize("counts", ["C20", "C16", "C20_7"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_fixed_15_majors(ncars, counts):
    """Fixed-work parity at the project's tolerances (objective 1e-7, x 1e-5), at the number of majors where these problems still allow it:
    see test_fixed_50_majors.  At 15 majors the oracle's own answer moves by at most 2.5e-14 (objective) and 1.2e-11 (x) under a 1e-15
    perturbation of x0, four to six decades below the tolerances.  C20_7 has a group of 7 breakpoints (ig_n = 0): the wave solver declines."""
    dobj, dx = fixed_majors(ncars, counts, 15)
    assert dobj <= 1e-7 and dx <= 1e-5


@pytest.mark.parametrize("counts", ["C20", "C16", "C20_7"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_fixed_50_majors(ncars, counts):
    """The benchmark's 50 majors.  Counts of majors and evaluations are exact (same_work).  Objective and x cannot agree to 1e-7 / 1e-5 here,
    and the kernels are not wrong: on these grids the quasi-Newton iteration from the identity start amplifies a perturbation a
    hundredfold per major from about major 20 on (the reduced Hessian has a condition number of 1.5e5).  The ORACLE, started from
    x0 (1 + 1e-15 N(0, 1)) instead of x0 = 1, differs from itself after 10 / 15 / 20 / 25 / 50 majors by up to 1.2e-14 / 2.5e-14 / 4.4e-12 /
    1.1e-3 / 3.3e-2 in the objective and 1.9e-14 / 1.2e-11 / 8.5e-8 / 1.1e-3 / 9.7e-3 in x (the nine cases, four draws; on the uniform
    grids B, M and M4b: 7e-11 .. 2e-9 in the objective at 50 majors, which is why tests/test_gpu_solve.py can ask for 1e-7).  Two
    implementations that round differently are two such starts.  Measured against the oracle on the device: 2.1e-4 .. 3.0e-2 in the
    objective and 2.3e-4 .. 1.1e-2 in x at 50 majors (at 15 majors: 6e-14 and 1e-11).  The bounds here, 1e-1 for the objective and 3e-2 for
    x, are three times the largest gap either measurement shows: they say that 50 majors made the same progress, no more.  The tight comparisons of the same kernels on the same grids are test_fixed_15_majors (per major) and
    test_solve_to_convergence (the identity start carried to the optimum, 60 .. 100 majors, objective to 1e-9)."""
    dobj, dx = fixed_majors(ncars, counts, 50)
    assert dobj <= 1e-1 and dx <= 3e-2


# -- g. degenerate grids -----------------------------------------------------------------------------------------------------------------
def stopping_rule_gap(spec, ref):
    """How far the objectives of two converged runs of a kincar problem may lie apart, from the stopping rule alone, per problem: the cost
    is a quadratic form, F = x'Hx / 2 with g = H x, so on A x = b  F - F* = pg'(Z'HZ)^-1 pg / 2 <= |pg|^2 / (2 lmin) with pg = Z'g the projected
    gradient and lmin the smallest eigenvalue of the reduced Hessian; a run ends at inform 0 with |pg| <= tolg = sqrt(eps^0.8) (1 +
    max(1 + |F|, |g|)) (oracle/sqp.c, NPSOL's rule).  Both runs end above F*, so they differ by at most that.  H, Z, F and g from the oracle."""
    import scipy.linalg
    H = orc.eval_batch(spec, np.eye(spec.nC), 2, nthreads=8)["g"]
    Z = scipy.linalg.null_space(orc.export_tables(spec)["A"])
    lmin = np.linalg.eigvalsh(Z.T @ (0.5 * (H + H.T)) @ Z)[0]
    assert lmin > 0
    g = orc.eval_batch(spec, ref["x"], 2)["g"]
    tolg = np.sqrt(np.finfo(np.float64).eps ** 0.8) * (1.0 + np.maximum(1.0 + np.abs(ref["objective"]), np.linalg.norm(g, axis=1)))
    return tolg ** 2 / (2.0 * lmin)


@pytest.mark.parametrize("hessian", [0, 1])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_interval_without_a_breakpoint(ncars, hessian):
    """C20_0: 19 breakpoint groups on 20 knot intervals; the coefficients of the empty interval are still determined (every basis function
    reaches into a neighbouring interval).  Neither the interval kernel nor the wave solver takes it: sqp_kernel.

    hessian = 1 meets the 1e-9 of test_solve_to_convergence.  hessian = 0 does not, and the kernel is not wrong: the objective gap to the
    oracle was measured at 1.9e-9 .. 2.3e-9 (first problem over 1e-9 of each of the three cases; F = 0.55 .. 0.96).  Both sides stop when
    the projected gradient meets NPSOL's rule, and what that rule leaves of the objective depends on the curvature: the empty interval
    lowers the smallest eigenvalue of the reduced Hessian from 0.143 (C20) to 0.034, and the rule's own bound (stopping_rule_gap) is
    1.5e-8 .. 3.6e-7 for these problems.  The 1e-9 of the other grids is what a superlinear iteration usually leaves under that rule, not
    what the rule promises.  The tolerance here is the rule's bound, computed per problem from the oracle alone.

    Feasibility, hessian = 0: |A x - b| was measured at 1.19e-8 and 1.29e-8 on the final acceleration row of one problem each (2 and 4
    outputs), over the 1e-8 of tests/test_gpu_solve.py; the oracle's own solutions reach 7.7e-9 on this grid.  The steps stay in null(A) to
    rounding only, and what 95 .. 128 majors leave behind scales with the row: these rows carry entries up to 1665 (20 / h^2 at the short
    end of the uneven knots) where the uniform grids of tests/test_gpu_solve.py have 640; relative to |A| |x| the residual is 3e-13.  The
    tolerance is 1e-8 scaled by that ratio of the rows, 2.6e-8: twice the measured gap."""
    name = f"K{ncars}-C20_0"
    p = plan(name)
    lo, up = cf.kincar_random_bounds(ncars, ug.NB_DEGEN)
    kern = p.solve_kernel(ug.NB_DEGEN, api.default_opts(hessian=hessian))
    print(f"{name} hessian {hessian}: {kern}")
    assert kern == "sqp_kernel"
    x, out = gpu_solve(p, lo, up, hessian=hessian)
    ref = orc_solve(name, lo, up, hessian=hessian)
    tol, feas_tol = None, 1e-8
    if hessian == 0:
        tol = stopping_rule_gap(p.spec, ref)
        feas_tol = 1e-8 * np.abs(orc.export_tables(p.spec)["A"]).max() / np.abs(orc.export_tables(cf.config_M())["A"]).max()
        print(f"  stopping rule's bound of the objective gap {tol}  feasibility tolerance {feas_tol:.2e}")
    check_optimum(p, x, out, ref, lo, obj_tol=tol, feas_tol=feas_tol)
    if hessian == 1:
        assert out["iters"].max() <= 5 and np.abs(out["iters"] - ref["iters"]).max() <= 1, (out["iters"], ref["iters"])


@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_singular_model_downgrades_to_the_identity_start(ncars):
    """C20_thin: intervals with one breakpoint leave the collocation model of the cost singular on null(A) (build_precond: precond_singular), and
    hessian = 1 must run as hessian = 0, like the oracle's fallback: the same majors as its own hessian = 0 run (within 1), dozens instead
    of the 3 of the preconditioned start.  x is not compared: the minimiser of a singular model is not unique."""
    name = f"K{ncars}-C20_thin"
    p = plan(name)
    lo, up = cf.kincar_random_bounds(ncars, ug.NB_DEGEN)
    print(f"{name}: hessian 1 {p.solve_kernel(ug.NB_DEGEN, api.default_opts(hessian=1))}, hessian 0 {p.solve_kernel(ug.NB_DEGEN, api.default_opts(hessian=0))}")
    x1, o1 = gpu_solve(p, lo, up, hessian=1)
    x0, o0 = gpu_solve(p, lo, up, hessian=0)
    ref = orc_solve(name, lo, up, hessian=1)
    check_optimum(p, x1, o1, ref, lo, compare_x=False)
    assert (o0["inform"] == 0).all()
    assert np.abs(o1["iters"] - o0["iters"]).max() <= 1, (o1["iters"], o0["iters"])
    assert o1["iters"].min() > 5                                  # (5: the most the preconditioned start may take, test_solve_to_convergence)


# -- h. Newton and QP modes --------------------------------------------------------------------------------------------------------------
_second = {}


def second_order(name, hessian):
    if (name, hessian) not in _second:
        p = plan(name)
        lo, up = ug.second_order_bounds(name, hessian)
        x, out = gpu_solve(p, lo, up, want_lambda=True, hessian=hessian)
        _second[(name, hessian)] = (p, lo, up, x, out, orc_solve(name, lo, up, hessian=hessian))
    return _second[(name, hessian)]


@pytest.mark.parametrize("hessian", [2, 3])
@pytest.mark.parametrize("name", ug.SECOND_ORDER)
def test_newton_and_qp_modes(name, hessian):
    """each mode against the oracle in the same mode (E8's two modes reach different local optima in the oracle: nothing is compared across
    modes).  The group colours of the structured model (`cover`, build_newton_tables) come from offsets of groups of 3 .. 6 breakpoints.

    Objective: 1e-9; in the Newton mode one problem of a batch may reach 1e-8, the rule of tests/test_gpu_newton.py::
    test_newton_solve_matches_oracle and for its reason: the augmented-Lagrangian passes end at a violation of up to 1e-8 (measured here
    with Plan.kkt: 1e-10 .. 3.8e-8), the two sides end a major apart on a few problems, and the objective follows the violation to first
    order through the multipliers.  Measured: O on C20, problem 8, 1.09e-9 (the next largest 8.8e-10); every other case and the whole QP
    mode below 1e-9."""
    p, lo, up, x, out, ref = second_order(name, hessian)
    print(f"{name} hessian {hessian}: {p.solve_kernel(lo.shape[0], api.default_opts(hessian=hessian))} majors {out['iters']} oracle {ref['iters']}")
    assert (out["inform"] == 0).all() and (ref["inform"] == 0).all(), (out["inform"], ref["inform"])
    assert np.abs(out["iters"] - ref["iters"]).max() <= 3, (out["iters"], ref["iters"])
    dobj = np.abs(out["objective"] - ref["objective"]) / np.maximum(1.0, np.abs(ref["objective"]))
    print(f"  objective gap {dobj}  x gap {np.abs(x - ref['x']).max():.2e}")
    if hessian == 2:
        assert (dobj <= 1e-8).all() and int((dobj > 1e-9).sum()) <= 1, dobj
    else:
        assert (dobj <= 1e-9).all(), dobj
    assert np.abs(x - ref["x"]).max() <= 1e-6 * max(1.0, np.abs(ref["x"]).max()), np.abs(x - ref["x"]).max()


@pytest.mark.parametrize("hessian", [2, 3])
def test_solved_obstacle_batch_passes_the_kkt_audit(hessian):
    """Plan.kkt on the points and multipliers of O on C20: stationarity at the threshold of tests/test_gpu_kkt.py::
    test_solved_batch_passes_the_audit, the linear rows to that test's 1e-9 rowscale + 1e-9 and the nonlinear
    rows to the 1e-8 (1 + |bound|) of tests/test_gpu_newton.py::_kkt"""
    p, lo, up, x, out, _ = second_order("O-C20", hessian)
    spec = p.spec
    res = p.kkt(dev(x), dev(lo), dev(up), dev(out["clambda"]))["res"].cpu().numpy()
    A = p.tables()["A"]
    nl0 = spec.nbounds - spec.nnlic - spec.nnltc - spec.nnlfc
    for i in range(x.shape[0]):
        lmax = res[i, 5]
        fin = np.concatenate([lo[i, nl0:], up[i, nl0:]]); fin = np.abs(fin[np.abs(fin) < 1e20])
        Lmax = fin.max(initial=0.0)
        rowscale_max = (np.abs(A).max(axis=1) * max(1.0, np.abs(x[i]).max())).max()
        print(f"problem {i}: res {res[i]}  stationarity {res[i, 0] / max(1.0, res[i, 1]):.2e}  |lambda| max {lmax:.2e}")
        assert res[i, 0] <= 2e-5 * max(1.0, res[i, 1]), (i, res[i])
        assert res[i, 2] <= 1e-9 * rowscale_max + 1e-9, (i, res[i])
        assert res[i, 3] <= 1e-8 * (1 + Lmax), (i, res[i])


# -- i. Plan.interp ----------------------------------------------------------------------------------------------------------------------
def test_interp_on_uneven_knots():
    """ntg_batch_interp == SplineInterp (restated in the oracle) on uneven knots: both ends, three interior knots, the breakpoint one ulp
    below a knot (it belongs to the interval before the knot) and 20 random times"""
    p = plan("K3-C20"); spec = p.spec
    rng = np.random.default_rng(21)
    nb = 5
    x = rng.normal(size=(nb, spec.nC))
    t0, t1 = float(spec.bps[0]), float(spec.bps[-1])
    kn = spec.knots[0]
    tulp = np.nextafter(kn[3], -np.inf)
    assert tulp in spec.bps
    times = np.concatenate([[t0, t1], kn[1:-1][:3], [tulp], rng.uniform(t0, t1, 20)])
    z = p.interp(dev(x), dev(times)).cpu().numpy()
    assert z.shape == (nb, len(times), spec.nz)
    dp = C.POINTER(C.c_double)
    ref = np.zeros_like(z)
    iz = np.concatenate([[0], np.cumsum(spec.maxderiv)]); iC = np.concatenate([[0], np.cumsum(spec.ncoef)])
    for b in range(nb):
        for o in range(spec.nout):
            kno = np.ascontiguousarray(spec.knots[o]); co = np.ascontiguousarray(x[b, iC[o]:iC[o + 1]])
            for ti, t in enumerate(times):
                f = np.zeros(spec.maxderiv[o])
                orc.lib().orc_spline_interp(f.ctypes.data_as(dp), C.c_double(float(t)), kno.ctypes.data_as(dp), int(spec.kninterv[o]),
                                            co.ctypes.data_as(dp), int(spec.ncoef[o]), int(spec.order[o]), int(spec.mult[o]), int(spec.maxderiv[o]))
                ref[b, ti, iz[o]:iz[o + 1]] = f
    assert rel(z, ref) <= 1e-13
