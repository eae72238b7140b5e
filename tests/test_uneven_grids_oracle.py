"""The oracle on the uneven shared grids of tests/uneven_grids.py: the conditions tests/test_gpu_uneven_grids.py relies on, asserted on the
CPU, so that a later change to the oracle cannot quietly empty the GPU tests (a solve that no longer converges, a fixed-work run that is no
longer regular in the sense of gpu_common.same_work, a `hessian = 1` that no longer falls back on the singular model).

What is pinned elsewhere: the basis blocks against scipy (tests/test_oracle_pgs.py), cost / gradient / rows / Jacobian / A / bounds against
the reference's own code, bit for bit (tests/test_oracle_vs_reference.py, fixtures ref_U20 / U16 / UO / UD8)."""
import numpy as np
import pytest

import orc
from ntg_amd import configs as cf
import uneven_grids as ug

_solved = {}


def solved(ncars, name, nb, **kw):
    key = (ncars, name, nb, tuple(sorted(kw.items())))
    if key not in _solved:
        spec = ug.kincar(ncars, name)
        lo, up = cf.kincar_random_bounds(ncars, nb)
        _solved[key] = orc.solve_batch(spec, lo, up, np.ones((nb, spec.nC)), orc.default_opts(**kw), nthreads=8)
    return _solved[key]


def test_grids_are_what_the_names_say():
    """breakpoints per knot interval as the oracle's own offsets group them: the count list, the end point in the last group, the one-ulp
    breakpoint of C20 still in the third interval"""
    for name, counts in ug.COUNTS.items():
        spec = ug.kincar(1, name) if name != "C8" else ug.E8()
        assert spec.nbps == sum(counts) + 1
        off = orc.export_tables(spec)["off"][0]
        got = np.bincount(off // (spec.order[0] - spec.mult[0]), minlength=len(counts))
        want = np.array(counts); want[-1] += 1
        assert np.array_equal(got, want), (name, got)
    kn, bps = ug.grid(ug.C20, 5.0, ulp=True)
    i = sum(ug.C20[:3]) - 1
    assert bps[i] < kn[3] and np.nextafter(bps[i], np.inf) == kn[3] and bps[i + 1] == kn[3]
    assert np.diff(kn)[0] / np.diff(kn)[-1] > 1.8          # the knots are far from uniform
    k2, b2 = ug.grid(ug.C20, 5.0, ulp=True)
    assert np.array_equal(kn, k2) and np.array_equal(bps, b2)


@pytest.mark.parametrize("name", ["C20", "C16", "C20_7", "C20_0"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_quasi_newton_modes_converge(ncars, name):
    """inform 0 from both starts; the preconditioned start needs at most 3 majors, the identity start dozens"""
    nb = ug.NB_DEGEN if name == "C20_0" else ug.NB_CONV
    r0, r1 = solved(ncars, name, nb, hessian=0), solved(ncars, name, nb, hessian=1)
    assert (r0["inform"] == 0).all() and (r1["inform"] == 0).all()
    assert r1["iters"].max() <= 3 and r0["iters"].min() > 3
    assert np.abs(r0["objective"] - r1["objective"]).max() <= 1e-9 * np.abs(r1["objective"]).max()


@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_singular_model_falls_back_to_the_identity_start(ncars):
    """C20_thin: the reduced Hessian model is singular, hessian = 1 is hessian = 0 (the same majors, 78 .. 96 of them)"""
    r0, r1 = solved(ncars, "C20_thin", ug.NB_DEGEN, hessian=0), solved(ncars, "C20_thin", ug.NB_DEGEN, hessian=1)
    assert (r0["inform"] == 0).all() and (r1["inform"] == 0).all()
    assert np.array_equal(r0["iters"], r1["iters"]) and r1["iters"].min() > 3     # (3: what the preconditioned start needs on the other lists)
    assert np.array_equal(r0["x"], r1["x"])


@pytest.mark.parametrize("itlim", [15, 50])
@pytest.mark.parametrize("name", ["C20", "C16", "C20_7"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_fixed_work_is_regular(ncars, name, itlim):
    """15 and 50 fixed majors: every problem ends at inform 4 after 2 itlim + 1 evaluations (31, 101) -- the whole batch is regular for
    gpu_common.same_work"""
    r = solved(ncars, name, ug.NB_FIXED, itlim=itlim, fixed_iters=1)
    assert (r["inform"] == 4).all() and (r["iters"] == itlim).all() and (r["nfev"] == 2 * itlim + 1).all()


@pytest.mark.parametrize("name", ["C20", "C16", "C20_7"])
@pytest.mark.parametrize("ncars", [1, 2, 3])
def test_fixed_work_amplifies_rounding_after_major_20(ncars, name):
    """Why the GPU tests compare fixed-work runs at 15 majors and not at 50 on these grids: the quasi-Newton iteration from the identity start
    amplifies a perturbation of x0 of 1e-15 to less than 1e-9 of x after 15 majors (measured: 1.2e-11), and to more than 1e-5 -- the
    tolerance of the fixed-work comparison -- after 50 (measured: 2.5e-4 .. 9.7e-3).  Two implementations that round differently are two
    such starts."""
    spec = ug.kincar(ncars, name)
    lo, up = cf.kincar_random_bounds(ncars, ug.NB_FIXED)
    x0 = np.ones((ug.NB_FIXED, spec.nC))
    x1 = x0 * (1.0 + 1e-15 * np.random.default_rng(0).normal(size=x0.shape))
    gap = {}
    for itlim in (15, 50):
        a = solved(ncars, name, ug.NB_FIXED, itlim=itlim, fixed_iters=1)
        b = orc.solve_batch(spec, lo, up, x1, orc.default_opts(itlim=itlim, fixed_iters=1), nthreads=8)
        gap[itlim] = np.abs(a["x"] - b["x"]).max() / np.abs(a["x"]).max()
    assert gap[15] <= 1e-9 and gap[50] > 1e-5, gap


@pytest.mark.parametrize("hessian", [2, 3])
@pytest.mark.parametrize("name", ug.SECOND_ORDER)
def test_newton_and_qp_modes_converge(name, hessian):
    spec = ug.ALL[name]()
    lo, up = ug.second_order_bounds(name, hessian)
    nb = lo.shape[0]
    r = orc.solve_batch(spec, lo, up, np.ones((nb, spec.nC)), orc.default_opts(hessian=hessian), nthreads=8)
    assert (r["inform"] == 0).all(), r["inform"]


@pytest.mark.parametrize("name", ["K1-C20", "K2-C16", "K1-C20_7", "K1-C20_0", "K1-C20_thin", "O-C20", "O-C16", "D8-C8", "E8-C8"])
def test_gradient_is_the_derivative_of_the_cost(name):
    """central difference of f, h = 1e-6, relative 1e-6, on every count list (independent of the reference: the interval lengths and the
    weights of the trapezoid rule enter f and g through different loops)"""
    spec = ug.ALL[name]()
    x = np.random.default_rng(17).normal(size=(1, spec.nC))
    g = orc.eval_batch(spec, x, 2)["g"][0]
    h = 1e-6
    cols = np.arange(0, spec.nC, max(1, spec.nC // 60))
    xp = np.repeat(x, len(cols), axis=0); xm = xp.copy()
    xp[np.arange(len(cols)), cols] += h; xm[np.arange(len(cols)), cols] -= h
    fd = (orc.eval_batch(spec, xp, 0)["f"] - orc.eval_batch(spec, xm, 0)["f"]) / (2 * h)
    assert np.abs(fd - g[cols]).max() <= 1e-6 * np.abs(g).max()
