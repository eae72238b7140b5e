"""-m gpu: the host-callback path of the drop-in with outputs of mixed order, mult and maxderiv (tests/hostpath_cases.py).

Every other plan of the suite has maxderiv 3 (5 for the quadrotor) on every output, so iz[o] = 3 o and d[o] is one number; here they are
not (MIX5: maxderiv 1,4,2,10,3, five basis classes; WIDE16: 16 outputs, nz = 64, mask bit 63).  Two routes, both against the oracle:

  through Python, on a Plan with family = -1 (NTG_FAM_HOST): tables() (basis_kernel, the class builder, linrows_kernel), bounds()
  (bounds_kernel) and interp() (basis_kernel at other times, interp_kernel);

  through tests/drivers/hostpath_drv.c linked against libntg_amd.so, compared with the SAME driver linked against the oracle's ABI library
  and run in the same test: npsolCostFunction / npsolConstraintFunction (hostz_kernel, hostcost_kernel, hostcon_kernel), SplineInterp,
  and ntg() on the solve cases.

Tolerances.  Basis blocks, A rows and interpolated values: the project's 1e-13 of max |ref| (tests/test_gpu_basis_eval.py), here per (output,
derivative) slice and per row, because tests/test_hostpath_oracle.py measures the oracle itself at 4.4e-16 of max |slice| against a 50-digit
evaluation -- under 1e-14 on every slice -- so nothing wider is called for.  F, G, C and J: the project's 1e-12 of max |ref|, G also per
output block and J per row.  Solves: those of test_vanderpol_dropin (equality rows) and test_linear_inequality_rows_dropin (range row).
Every figure is measured against the oracle, never against the kernels' own output.  Every driver run is one subprocess with a time limit;
no step is retried.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostpath_cases as hc
import orc
from gpu_common import dev
from ntg_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "tests", "drivers", "hostpath_drv.c")
TOL_BASIS = 1e-13      # blk, A, interp, Z: see the module docstring
TOL_EVAL = 1e-12       # F, G, C, J
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the one driver source linked against the product and against the oracle's ABI library"""
    d = tmp_path_factory.mktemp("hostpath_drv")
    exes = {}
    for lib, libdir in (("ntg_amd", os.path.join(ROOT, "ntg_amd")), ("orc_ntg", os.path.join(ROOT, "oracle"))):
        exes[lib] = d / ("hostpath_drv_" + lib)
        subprocess.check_call(["gcc", "-O1", "-I", os.path.join(ROOT, "include"), DRV, "-o", str(exes[lib]), "-L", libdir, "-l" + lib, "-lm",
                               "-Wl,-rpath," + libdir])
    return d, exes


_cache = {}


def both(drivers, key, mode, files, options=(), check=True):
    """the driver under the oracle, then under the product: (oracle stdout, product stdout); one subprocess each, one after the other"""
    if key not in _cache:
        d, exes = drivers
        outs = []
        for lib in ("orc_ntg", "ntg_amd"):
            out = subprocess.run([str(exes[lib]), mode, *[str(f) for f in files], *options], capture_output=True, text=True, timeout=120)
            assert out.returncode >= 0 and (not check or out.returncode == 0), (lib, out.returncode, out.stderr[-2000:], out.stdout[-2000:])
            outs.append(out)
        _cache[key] = outs
    return _cache[key]


def case_file(drivers, name):
    case = hc.CASES[name]()
    return case, hc.write(case, drivers[0] / (name + ".txt"))


def spline_interp_ref(spec, x, o, t):
    L = orc.lib()
    L.orc_spline_interp.argtypes = [dp, C.c_double, dp, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int]
    iC = int(np.sum(spec.ncoef[:o]))
    f = np.zeros(spec.maxderiv[o]); kn = np.ascontiguousarray(spec.knots[o], dtype=np.float64)
    cf = np.ascontiguousarray(x[iC:iC + spec.ncoef[o]], dtype=np.float64)
    L.orc_spline_interp(f.ctypes.data_as(dp), float(t), kn.ctypes.data_as(dp), spec.kninterv[o], cf.ctypes.data_as(dp), spec.ncoef[o],
                        spec.order[o], spec.mult[o], spec.maxderiv[o])
    return f


def within(got, ref, tol, what):
    """max |got - ref| <= tol max |ref|, with the figure printed before it is asserted"""
    got = np.asarray(got, dtype=float); ref = np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    if err > 0.1 * tol * scale:
        print(what, "max|d| %.3e of max|ref| %.3e = %.3e" % (err, scale, err / max(scale, 1e-300)))
    assert err <= tol * scale, (what, err, scale)
    return err / max(scale, 1e-300)


_plans = {}


def plan_of(name):
    """a Plan on the case's spec with family = -1: plan creation, tables(), bounds() and interp() carry no refusal for host-callback plans"""
    if name not in _plans:
        case = hc.CASES[name]()
        assert case.spec.family == -1
        _plans[name] = (case, api.Plan(case.spec, 0))
    return _plans[name]


# ---------------------------------------------------------------- through Python ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIX5", "WIDE16"])
def test_tables_of_mixed_outputs(name):
    """tables(): off exact; blk per (output, derivative) slice and every row of A within 1e-13 of the oracle's (the project's figure, see the
    module docstring for why not wider); A with the oracle's non-zero pattern exactly.  A wrong d[o] or k in basis_kernel's output stride
    or in the class builder's blk offsets moves a slice; a wrong iz[o] + l or cls_blk in linrows_kernel moves a row of A."""
    case, plan = plan_of(name)
    sp = case.spec
    ref = orc.export_tables(sp, case.lower, case.upper)
    t = plan.tables()
    assert np.array_equal(t["off"], ref["off"])
    pos, worst = 0, 0.0
    for o, (k, d) in enumerate(zip(sp.order, sp.maxderiv)):
        n = sp.nbps * k * d
        g = t["blk"][pos:pos + n].reshape(sp.nbps, k, d); r = ref["blk"][pos:pos + n].reshape(sp.nbps, k, d); pos += n
        for rr in range(d):
            worst = max(worst, within(g[:, :, rr], r[:, :, rr], TOL_BASIS, "%s blk output %d derivative %d" % (name, o, rr)))
    assert pos == len(t["blk"]) == len(ref["blk"])
    assert t["A"].shape == ref["A"].shape == (sp.nclin, sp.nC)
    assert np.array_equal(t["A"] != 0, ref["A"] != 0)
    for r in range(sp.nclin):
        worst = max(worst, within(t["A"][r], ref["A"][r], TOL_BASIS, "%s A row %d" % (name, r)))
    print(name, "tables: worst slice / row error relative to its maximum %.3e" % worst)


def test_bounds_of_mixed_outputs():
    """bounds(): exact against the reference's bounds() on MIX5 (tests/golden/ref_H.npz) and against the oracle on both cases"""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_H.npz")))
    for name in ("MIX5", "WIDE16"):
        case, plan = plan_of(name)
        ref = orc.export_tables(case.spec, case.lower, case.upper)
        bl, bu = plan.bounds(dev(case.lower[None]), dev(case.upper[None]))
        bl = bl.cpu().numpy()[0]; bu = bu.cpu().numpy()[0]
        assert np.array_equal(bl, ref["bl"]) and np.array_equal(bu, ref["bu"])
        if name == "MIX5":
            assert np.array_equal(bl, g["bl"]) and np.array_equal(bu, g["bu"])


@pytest.mark.parametrize("name", ["MIX5", "WIDE16"])
def test_interp_of_mixed_outputs(name):
    """interp(): 5 random coefficient rows at both ends, three interior knots each of outputs 0 and 2 and 20 random times, against
    orc_spline_interp of every output with its own maxderiv, per (output, derivative) slice at 1e-13 (module docstring).  A wrong iz[o],
    d[o] or class base in interp_kernel moves a slice."""
    case, plan = plan_of(name)
    sp = case.spec
    x = np.random.default_rng(17).normal(size=(5, sp.nC))
    z = plan.interp(dev(x), dev(case.times)).cpu().numpy()
    assert z.shape == (5, len(case.times), sp.nz)
    iz = np.concatenate([[0], np.cumsum(sp.maxderiv)])
    worst = 0.0
    for o in range(sp.nout):
        ref = np.array([[spline_interp_ref(sp, x[b], o, t) for t in case.times] for b in range(5)])      # [5, ntimes, d_o]
        for r in range(sp.maxderiv[o]):
            worst = max(worst, within(z[:, :, iz[o] + r], ref[:, :, r], TOL_BASIS, "%s interp output %d derivative %d" % (name, o, r)))
    print(name, "interp: worst slice error relative to its maximum %.3e" % worst)


# ---------------------------------------------------------------- through the driver: evaluation ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIX5", "WIDE16"])
def test_eval_of_mixed_outputs_through_the_driver(drivers, name):
    """npsolCostFunction / npsolConstraintFunction on the case's three points (N(0,1), 3 N(0,1), all ones), product against oracle:
      F, G, C within 1e-12 of max |ref|; G also per output block of coefficients (a wrong tavrow[iz + r], chrow[chb + r] or oinfo entry in
      hostcost_kernel's generic branch moves one block, and the order-10 output's scale must not hide it); J with the oracle's non-zero
      pattern and every row within 1e-12 (hostcon_kernel: dc[row][iz[o] + r], chrow[cc * NTG_MAX_ORDER + r]); mode 0's F and mode 1's G equal
      mode 2's; the caller's rows [ncnln, ldJ) of cJac untouched; the Z lines -- what the trajectory cost callback was handed, hostz_kernel's
      Z[iz[o] P + d[o] bp + r] under its 64-bit mask -- and the INTERP lines (SplineInterp) per (output, derivative) slice at 1e-13."""
    case, f = case_file(drivers, name)
    sp = case.spec
    o_out, p_out = both(drivers, ("eval", name), "eval", [f])
    ref = hc.parse_eval(o_out.stdout, case); got = hc.parse_eval(p_out.stdout, case)
    assert len(ref) == len(got) == 3
    iC = np.concatenate([[0], np.cumsum(sp.ncoef)])
    for pt, (g, r) in enumerate(zip(got, ref)):
        tag = "%s point %d " % (name, pt)
        assert abs(g["F"] - r["F"]) <= TOL_EVAL * abs(r["F"]), (tag, g["F"], r["F"])
        within(g["G"], r["G"], TOL_EVAL, tag + "G")
        for o in range(sp.nout):
            within(g["G"][iC[o]:iC[o + 1]], r["G"][iC[o]:iC[o + 1]], TOL_EVAL, tag + "G block of output %d" % o)
        within(g["C"], r["C"], TOL_EVAL, tag + "C")
        assert g["F0"] == g["F"] and np.array_equal(g["G1"], g["G"])
        assert g["J"].shape == (sp.ncnln + 2, sp.nC)
        assert np.all(g["J"][sp.ncnln:] == -7.25) and np.all(r["J"][sp.ncnln:] == -7.25)
        Jg, Jr = g["J"][:sp.ncnln], r["J"][:sp.ncnln]
        assert np.array_equal(Jg != 0, Jr != 0)
        within(Jg, Jr, TOL_EVAL, tag + "J")
        for row in range(sp.ncnln):
            within(Jg[row], Jr[row], TOL_EVAL, tag + "J row %d" % row)
        assert g["Z"].shape == r["Z"].shape == (sp.nbps, len(sp.tcostav))
    # a slice is one (output, derivative) over the breakpoints (times) and the three points together: at the all-ones point every derivative
    # is rounding noise around 0 on both sides, and only the other two points say how large the slice is
    for j, (o, d) in enumerate(sp.tcostav):
        within(np.stack([g["Z"][:, j] for g in got]), np.stack([r["Z"][:, j] for r in ref]), TOL_BASIS, "%s Z of (%d, %d)" % (name, o, d))
    for o in range(sp.nout):
        for d in range(sp.maxderiv[o]):
            within(np.stack([g["INTERP"][o][:, d] for g in got]), np.stack([r["INTERP"][o][:, d] for r in ref]), TOL_BASIS,
                   "%s INTERP output %d derivative %d" % (name, o, d))


# ---------------------------------------------------------------- through the driver: solves ----------------------------------------------------------------
def solved(drivers, name, mode):
    """(case, oracle result, product result) of ntg() on the case; SOLVE3 in the default mode is the first call of the sequence run"""
    if (name, mode) == ("SOLVE3", "default"):
        c3, f3 = case_file(drivers, "SOLVE3"); _, f2 = case_file(drivers, "SOLVE2")
        o_out, p_out = both(drivers, ("sequence",), "sequence", [f3, f2])
        return c3, hc.parse_solve(o_out.stdout)[0], hc.parse_solve(p_out.stdout)[0]
    case, f = case_file(drivers, name)
    o_out, p_out = both(drivers, ("solve", name, mode), "solve", [f], hc.HESSIAN_MODES[mode], check=False)
    ro, rp = hc.parse_solve(o_out.stdout), hc.parse_solve(p_out.stdout)
    assert len(ro) == 1 and len(rp) == 1, p_out.stderr[-2000:] + p_out.stdout[-2000:]
    assert o_out.returncode == ro[0]["inform"] and p_out.returncode == rp[0]["inform"]
    return case, ro[0], rp[0]


@pytest.mark.parametrize("mode", list(hc.HESSIAN_MODES))
def test_solve_mixed_outputs(drivers, mode):
    """ntg() on SOLVE3 (orders 4,6,5, mult 2,3,3, maxderiv 2,4,3, equality rows), from coef = 0.5: the oracle's inform, the objective within
    1e-9 and the coefficients within 1e-6 of the oracle's (test_vanderpol_dropin's tolerances)"""
    case, ref, got = solved(drivers, "SOLVE3", mode)
    print("SOLVE3", mode, "product", got["inform"], repr(got["objective"]), "| oracle", ref["inform"], repr(ref["objective"]),
          "| max |dx| %.3e" % np.abs(got["x"] - ref["x"]).max())
    assert ref["inform"] == 0 and got["inform"] == ref["inform"]
    assert abs(got["objective"] - ref["objective"]) <= 1e-9
    np.testing.assert_allclose(got["x"], ref["x"], rtol=0, atol=1e-6)
    assert got["istate"] == ref["istate"] == [3] * case.spec.nclin


@pytest.mark.parametrize("mode", list(hc.HESSIAN_MODES))
def test_solve_mixed_outputs_with_a_range_row(drivers, mode):
    """ntg() on SOLVE3R (SOLVE3 plus z_0 + 0.5 z_1' + z_2 in [LO_R, UP_R] at every breakpoint, active at the optimum): the oracle's inform,
    the objective within 1e-7 max(1, |F|), the coefficients within 1e-5 of max |x|, ISTATE of the linear rows equal to the oracle's
    (test_linear_inequality_rows_dropin's tolerances)"""
    case, ref, got = solved(drivers, "SOLVE3R", mode)
    print("SOLVE3R", mode, "product", got["inform"], repr(got["objective"]), "| oracle", ref["inform"], repr(ref["objective"]),
          "| max |dx| %.3e" % np.abs(got["x"] - ref["x"]).max())
    assert ref["inform"] == 0 and got["inform"] == ref["inform"]
    assert abs(got["objective"] - ref["objective"]) <= 1e-7 * max(1.0, abs(ref["objective"]))
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-5 * np.abs(ref["x"]).max()
    assert got["istate"] == ref["istate"]
    assert any(s in (1, 2) for s in got["istate"])


def test_sequence_of_shapes_in_one_process(drivers):
    """ntg() on SOLVE3, SOLVE2 (another nout, nz, nC and row count) and SOLVE3 again in one process: every call sizes its Z and Jacobian
    buffers from its own shape and reaches its oracle optimum; the third result equals the first bit for bit"""
    c3, f3 = case_file(drivers, "SOLVE3"); c2, f2 = case_file(drivers, "SOLVE2")
    o_out, p_out = both(drivers, ("sequence",), "sequence", [f3, f2])
    ref = hc.parse_solve(o_out.stdout); got = hc.parse_solve(p_out.stdout)
    assert len(ref) == len(got) == 3
    for g, r in zip(got, ref):
        assert r["inform"] == 0 and g["inform"] == 0
        assert abs(g["objective"] - r["objective"]) <= 1e-9
        np.testing.assert_allclose(g["x"], r["x"], rtol=0, atol=1e-6)
    assert len(got[0]["x"]) == c3.spec.nC and len(got[1]["x"]) == c2.spec.nC and c3.spec.nC != c2.spec.nC
    assert np.array_equal(got[0]["x"], got[2]["x"]) and got[0]["objective"] == got[2]["objective"] and got[0]["istate"] == got[2]["istate"]
