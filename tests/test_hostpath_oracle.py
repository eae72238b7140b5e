"""The host-callback path with outputs of mixed order, mult and maxderiv (tests/hostpath_cases.py), on the CPU: what the oracle says about
those problems is pinned here, so that tests/test_gpu_hostpath.py can compare the product with it.

  * the oracle's A, bl, bu and updateZ against the reference's own code on MIX5 (tests/golden/ref_H.npz), bit for bit
  * the oracle's basis blocks against an independent evaluation (mpmath at 50 digits, else scipy): the measured error of the oracle,
    which the GPU tolerances are stated against
  * G and J of tests/drivers/hostpath_drv.c (linked against the oracle's ABI library) against central differences of its own F and C
  * what the trajectory cost callback is handed against SplineInterp at the breakpoints, bit for bit
  * the solve cases: inform 0 in both Hessian modes, equal objectives, SOLVE3R's range row active
  * the driver links against the product library (it needs a GPU to run there)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostpath_cases as hc
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DRV = os.path.join(ROOT, "tests", "drivers", "hostpath_drv.c")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
H_FD = 1e-6            # step of the central differences, as in test_gradient_finite_difference


def build_driver(tmp, libdir, lib, extra=()):
    exe = tmp / ("hostpath_drv_" + lib)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), DRV, "-o", str(exe), "-L", libdir, "-l" + lib, "-lm",
                           "-Wl,-rpath," + libdir] + list(extra))
    return exe


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    orc.build()
    return build_driver(tmp_path_factory.mktemp("hostpath"), os.path.join(ROOT, "oracle"), "orc_ntg")


def fd_points(case):
    """the case's points, then x0 +- h e_j for every 3rd coefficient j (F and C only), x0 = the first point"""
    x0 = case.points[0]
    js = list(range(0, case.spec.nC, 3))
    extra = []
    for j in js:
        for s in (+1.0, -1.0):
            x = x0.copy(); x[j] += s * H_FD; extra.append(x)
    pts = np.vstack([case.points, np.array(extra)])
    return js, pts, np.concatenate([np.ones(len(case.points), dtype=int), np.zeros(len(extra), dtype=int)])


_eval_cache = {}


def eval_case(drv, name, tmp_path_factory):
    """one run of the driver's eval mode per case: the case's three points in full, then the finite-difference points"""
    if name not in _eval_cache:
        case = hc.CASES[name]()
        js, pts, full = fd_points(case)
        f = hc.write(case, tmp_path_factory.mktemp(name) / "problem.txt", pts, full)
        out = subprocess.run([str(drv), "eval", str(f)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr + out.stdout[-2000:]
        _eval_cache[name] = (case, js, hc.parse_eval(out.stdout, case))
    return _eval_cache[name]


def spline_interp(spec, x, o, t):
    """orc_spline_interp of output o with its own maxderiv"""
    L = orc.lib()
    L.orc_spline_interp.argtypes = [dp, C.c_double, dp, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int]
    iC = int(np.sum(spec.ncoef[:o]))
    f = np.zeros(spec.maxderiv[o]); kn = np.ascontiguousarray(spec.knots[o], dtype=np.float64)
    cf = np.ascontiguousarray(x[iC:iC + spec.ncoef[o]], dtype=np.float64)
    L.orc_spline_interp(f.ctypes.data_as(dp), float(t), kn.ctypes.data_as(dp), spec.kninterv[o], cf.ctypes.data_as(dp), spec.ncoef[o],
                        spec.order[o], spec.mult[o], spec.maxderiv[o])
    return f


def blocks(spec, blk):
    """the flat block table as one [P, k_o, d_o] array per output"""
    out, pos = [], 0
    for k, d in zip(spec.order, spec.maxderiv):
        out.append(blk[pos:pos + spec.nbps * k * d].reshape(spec.nbps, k, d)); pos += spec.nbps * k * d
    return out


# ---------------------------------------------------------------- the reference's own code ----------------------------------------------------------------
def test_oracle_matches_the_mixed_layout_fixture():
    """A, bl, bu and Z (orc_updateZ, each of the six lists on a fresh Z) of MIX5 are bit-equal to what the reference's LinearConstraintsMatrix,
    bounds and updateZ gave (tests/golden/ref_H.npz): iZ, iz and iC with unequal maxderiv are the reference's, not the oracle's reading of them"""
    case = hc.CASES["MIX5"](); spec = case.spec
    g = dict(np.load(os.path.join(GOLD, "ref_H.npz")))
    tab = orc.export_tables(spec, case.lower, case.upper)
    assert np.array_equal(tab["blk"], g["blk"]) and np.array_equal(tab["off"], g["off"])
    assert np.array_equal(g["x"], case.points)
    assert np.array_equal(tab["A"], g["A"]) and g["A"].shape == (spec.nclin, spec.nC)
    assert np.array_equal(tab["bl"], g["bl"]) and np.array_equal(tab["bu"], g["bu"])
    L = orc.lib()
    cs = orc.CSpec(spec)
    L.orc_colloc_make.restype = C.c_void_p
    L.orc_colloc_make.argtypes = [C.c_int, C.POINTER(dp), ip, dp, C.c_int, ip, ip, ip]
    L.orc_updateZ.argtypes = [dp, C.c_void_p, dp, C.POINTER(orc.AVc), C.c_int, C.c_int]
    L.orc_colloc_free.argtypes = [C.c_void_p]
    cc = L.orc_colloc_make(spec.nout, cs.c.knots, cs.c.kninterv, cs.c.bps, spec.nbps, cs.c.maxderiv, cs.c.order, cs.c.mult)
    try:
        for b, x in enumerate(case.points):
            xb = np.ascontiguousarray(x)
            for j, (nm, typ) in enumerate(zip(hc.SLOTS, (0, 1, 2, 0, 1, 2))):
                lst = list(getattr(spec, nm))
                av = (orc.AVc * len(lst))(*[orc.AVc(o, d) for o, d in lst])
                Z = np.zeros(spec.nz * spec.nbps)
                L.orc_updateZ(Z.ctypes.data_as(dp), cc, xb.ctypes.data_as(dp), av, len(lst), typ)
                assert np.array_equal(Z, g["Z"][b, j]), (b, nm)
                assert np.count_nonzero(Z) > 0
    finally:
        L.orc_colloc_free(cc)


# ---------------------------------------------------------------- the basis, independently ----------------------------------------------------------------
def independent_basis(knots, k, m, x, nder):
    """D^r B_i(x), r < nder, of the k B-splines of order k that do not vanish on x's interval of the augmented knots (first and last break k
    times, interior breaks k - m times): Cox - de Boor for the values, the difference formula for the derivatives, right-continuous, the last
    interval at the right end.  Returns ([k, nder] as floats, index of the first of them).  mpmath at 50 digits where it imports, else scipy."""
    t = [knots[0]] * k + [kn for kn in knots[1:-1] for _ in range(k - m)] + [knots[-1]] * k
    n = (len(knots) - 1) * (k - m) + m
    assert len(t) == n + k
    real = [i for i in range(k - 1, n) if t[i] < t[i + 1]]
    left = max(real) if x >= t[-1] else max(i for i in real if t[i] <= x)
    try:
        import mpmath as mp
    except ImportError:
        from scipy.interpolate import BSpline
        out = np.zeros((k, nder))
        for q in range(k):
            c = np.zeros(n); c[left - k + 1 + q] = 1.0
            for r in range(nder):
                out[q, r] = BSpline(np.array(t, dtype=float), c, k - 1)(x, nu=r)
        return out, left - k + 1
    with mp.workdps(50):
        tt = [mp.mpf(float(v)) for v in t]; xx = mp.mpf(float(x))
        memo = {}

        def N(i, j, r):
            key = (i, j, r)      # B_{i,j} lives on t[i .. i + j]: inside the knot vector for every (i, j) the recursion reaches
            if key in memo:
                return memo[key]
            if j == 1:
                v = mp.mpf(1 if (r == 0 and i == left) else 0)
            else:
                d1 = tt[i + j - 1] - tt[i]; d2 = tt[i + j] - tt[i + 1]
                if r == 0:
                    v = (((xx - tt[i]) / d1) * N(i, j - 1, 0) if d1 != 0 else 0) + (((tt[i + j] - xx) / d2) * N(i + 1, j - 1, 0) if d2 != 0 else 0)
                else:
                    v = (j - 1) * ((N(i, j - 1, r - 1) / d1 if d1 != 0 else 0) - (N(i + 1, j - 1, r - 1) / d2 if d2 != 0 else 0))
            memo[key] = v
            return v
        out = np.array([[float(N(left - k + 1 + q, k, r)) for r in range(nder)] for q in range(k)])
    return out, left - k + 1


def basis_slice_errors(spec, blk, off):
    """max |blk - independent| / max |independent| per (output, derivative) slice over all breakpoints and block columns; off must be exact"""
    errs = {}
    for o, B in enumerate(blocks(spec, blk)):
        ref = np.zeros_like(B)
        for i, x in enumerate(spec.bps):
            ref[i], first = independent_basis([float(v) for v in spec.knots[o]], spec.order[o], spec.mult[o], float(x), spec.maxderiv[o])
            assert first == off[o, i], (o, i)
        for r in range(spec.maxderiv[o]):
            errs[(o, r)] = float(np.abs(B[:, :, r] - ref[:, :, r]).max() / np.abs(ref[:, :, r]).max())
    return errs


def test_oracle_basis_against_an_independent_evaluation():
    """The oracle's basis blocks of MIX5 (orders 4,7,2,10,5, mult 1,4,0,9,3, every derivative up to maxderiv 1,4,2,10,3, uneven knots, four
    breakpoints exactly on interior knots) against de Boor's recursion in 50-digit arithmetic, per (output, derivative) slice,
    max |d| / max |slice|.  Measured with mpmath 1.3.0: the worst slice is (output 3, derivative 0) at 4.441e-16; the worst slice per output is
    2.2e-16, 3.3e-16, 1.1e-16, 4.4e-16, 3.3e-16 -- the 9th derivative of the order-10 output included.  So the oracle itself is under 1e-14
    on every slice, and tests/test_gpu_hostpath.py compares the product with it at the project's 1e-13 (tests/test_gpu_basis_eval.py).
    The assertion keeps that premise true."""
    spec = hc.CASES["MIX5"]().spec
    tab = orc.export_tables(spec)
    errs = basis_slice_errors(spec, tab["blk"], tab["off"])
    worst = max(errs, key=errs.get)
    print("oracle basis vs independent evaluation: worst slice (output %d, derivative %d) %.3e; per output %s"
          % (worst[0], worst[1], errs[worst], ["%.1e" % max(v for (o, r), v in errs.items() if o == oo) for oo in range(spec.nout)]))
    assert errs[worst] < 1e-14


# ---------------------------------------------------------------- the driver on the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIX5", "WIDE16"])
def test_driver_derivatives_against_finite_differences(drv, name, tmp_path_factory):
    """G and J of the driver at the first point against central differences of its own F and C in every 3rd coefficient (h = 1e-6, the
    tolerance of test_gradient_finite_difference): the callbacks' df / dc and the oracle's assembly agree for unequal maxderiv.  Also here:
    mode 0 and mode 1 give mode 2's F and G, and the caller's rows [ncnln, ldJ) of cJac stay untouched."""
    case, js, pts = eval_case(drv, name, tmp_path_factory)
    sp = case.spec
    base = pts[0]; rest = pts[len(case.points):]
    assert base["J"].shape == (sp.ncnln + 2, sp.nC)
    for e, j in enumerate(js):
        ep, em = rest[2 * e], rest[2 * e + 1]
        fd = (ep["F0"] - em["F0"]) / (2 * H_FD)
        assert abs(fd - base["G"][j]) <= 1e-5 * max(1.0, abs(fd)), (j, fd, base["G"][j])
        fdc = (ep["C0"] - em["C0"]) / (2 * H_FD)
        np.testing.assert_allclose(base["J"][:sp.ncnln, j], fdc, rtol=0, atol=1e-5 * max(1.0, np.abs(fdc).max()))
    for p in pts[:len(case.points)]:
        assert p["F0"] == p["F"] and np.array_equal(p["G1"], p["G"])
        assert np.all(p["J"][sp.ncnln:] == -7.25)
        assert np.count_nonzero(p["G"]) == sp.nC and np.isfinite(p["J"]).all() and np.isfinite(p["C"]).all()


@pytest.mark.parametrize("name", ["MIX5", "WIDE16"])
def test_callback_is_handed_the_interpolated_values(drv, name, tmp_path_factory):
    """what the trajectory cost callback is handed for its active variables at every breakpoint (the driver's Z lines) equals
    orc_spline_interp of that output at that breakpoint, bit for bit: zp[o] points at the right maxderiv-strided place of Z for every
    output, and the driver's own INTERP lines are those values too"""
    case, js, pts = eval_case(drv, name, tmp_path_factory)
    sp = case.spec
    for p, x in zip(pts[:len(case.points)], case.points):
        assert p["Z"].shape == (sp.nbps, len(sp.tcostav))
        for i, t in enumerate(sp.bps):
            vals = {o: spline_interp(sp, x, o, t) for o in {o for o, _ in sp.tcostav}}
            assert np.array_equal(p["Z"][i], np.array([vals[o][r] for o, r in sp.tcostav])), i
        for o in range(sp.nout):
            assert p["INTERP"][o].shape == (len(case.times), sp.maxderiv[o])
            assert np.array_equal(p["INTERP"][o], np.stack([spline_interp(sp, x, o, t) for t in case.times]))


_solve_cache = {}


def solve_case(drv, name, mode, tmp_path_factory):
    if (name, mode) not in _solve_cache:
        case = hc.CASES[name]()
        f = hc.write(case, tmp_path_factory.mktemp(name + mode) / "problem.txt")
        out = subprocess.run([str(drv), "solve", str(f), *hc.HESSIAN_MODES[mode]], capture_output=True, text=True, timeout=120)
        res = hc.parse_solve(out.stdout)
        assert len(res) == 1 and out.returncode == res[0]["inform"], out.stderr + out.stdout[-2000:]
        _solve_cache[(name, mode)] = (case, res[0])
    return _solve_cache[(name, mode)]


@pytest.mark.parametrize("name", ["SOLVE3", "SOLVE3R", "SOLVE2"])
def test_solve_cases_converge_in_both_modes(drv, name, tmp_path_factory):
    """inform 0 from coef = 0.5 with the default options and with "hessian colloc", the two objectives within 1e-9 relative: the optimum
    the product is compared with exists and does not depend on the mode"""
    case, a = solve_case(drv, name, "default", tmp_path_factory)
    _, b = solve_case(drv, name, "colloc", tmp_path_factory)
    print(name, "objective default / colloc", repr(a["objective"]), repr(b["objective"]))
    assert a["inform"] == 0 and b["inform"] == 0
    assert abs(a["objective"] - b["objective"]) <= 1e-9 * abs(a["objective"])
    assert np.abs(a["x"] - b["x"]).max() <= 1e-4 * np.abs(a["x"]).max()
    sp = case.spec
    assert len(a["istate"]) == sp.nclin and a["istate"] == b["istate"]
    assert a["istate"][:sp.nlic] == [3] * sp.nlic and a["istate"][-sp.nlfc:] == [3] * sp.nlfc      # the pinned ends are equality rows


@pytest.mark.parametrize("mode", list(hc.HESSIAN_MODES))
def test_range_row_is_active(drv, mode, tmp_path_factory):
    """SOLVE3R's range row costs something: the objective exceeds SOLVE3's by more than 1e-6 relative, at least one of its rows sits at a
    bound, every row is inside [LO_R, UP_R] -- and SOLVE3's own optimum is outside it"""
    case, r = solve_case(drv, "SOLVE3R", mode, tmp_path_factory)
    free_case, free = solve_case(drv, "SOLVE3", mode, tmp_path_factory)
    sp = case.spec
    assert r["objective"] > free["objective"] * (1 + 1e-6)
    rows_state = r["istate"][sp.nlic:sp.nlic + sp.nbps]
    assert any(s in (1, 2) for s in rows_state), rows_state
    A = orc.export_tables(sp, case.lower, case.upper)["A"][sp.nlic:sp.nlic + sp.nbps]
    row = A @ r["x"]; row_free = A @ free["x"]
    assert row.min() >= hc.LO_R - 1e-7 and row.max() <= hc.UP_R + 1e-7
    assert row_free.max() > hc.UP_R + 1e-3 and row_free[0] > hc.LO_R and row_free[-1] < hc.UP_R
    assert all(abs(row[i] - (hc.LO_R if s == 1 else hc.UP_R)) <= 1e-6 for i, s in enumerate(rows_state) if s in (1, 2))


def test_sequence_gives_the_first_result_again(drv, tmp_path_factory):
    """ntg() on SOLVE3, SOLVE2 (another nout, nz, nC and row count) and SOLVE3 again in one process: each call reaches its own optimum, the
    third result equals the first bit for bit"""
    d = tmp_path_factory.mktemp("sequence")
    f3 = hc.write(hc.CASES["SOLVE3"](), d / "solve3.txt"); f2 = hc.write(hc.CASES["SOLVE2"](), d / "solve2.txt")
    out = subprocess.run([str(drv), "sequence", str(f3), str(f2)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout[-2000:]
    res = hc.parse_solve(out.stdout)
    assert len(res) == 3 and [r["inform"] for r in res] == [0, 0, 0]
    assert res[0]["objective"] == solve_case(drv, "SOLVE3", "default", tmp_path_factory)[1]["objective"]
    assert res[1]["objective"] == solve_case(drv, "SOLVE2", "default", tmp_path_factory)[1]["objective"]
    assert len(res[0]["x"]) != len(res[1]["x"])
    assert np.array_equal(res[0]["x"], res[2]["x"]) and res[0]["objective"] == res[2]["objective"] and res[0]["istate"] == res[2]["istate"]


def test_refusals_of_the_exported_callbacks():
    """the oracle's npsolCostFunction / npsolConstraintFunction refuse like the product's: nstate = -1 / mode = -1 without a current problem"""
    orc.build()
    L = C.CDLL(os.path.join(ROOT, "oracle", "liborc_ntg.so"))
    mode, n, nstate, nc, ldJ, needc = C.c_int(2), C.c_int(3), C.c_int(1), C.c_int(0), C.c_int(1), C.c_int(0)
    x = (C.c_double * 3)(); f = C.c_double(0)
    L.npsolCostFunction(C.byref(mode), C.byref(n), x, C.byref(f), x, C.byref(nstate))
    assert nstate.value == -1
    L.npsolConstraintFunction(C.byref(mode), C.byref(nc), C.byref(n), C.byref(ldJ), C.byref(needc), x, x, x, C.byref(nstate))
    assert mode.value == -1


# ---------------------------------------------------------------- the product library: link only ----------------------------------------------------------------
def test_driver_links_against_the_product_library(tmp_path):
    """tests/drivers/hostpath_drv.c, written against include/ntg.h and include/ntg_amd.h only, links against libntg_amd.so with
    --no-undefined (it needs a GPU to run there: tests/test_gpu_hostpath.py), and the library exports every entry point it calls"""
    lib = os.path.join(ROOT, "ntg_amd", "libntg_amd.so")
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    exe = build_driver(tmp_path, os.path.join(ROOT, "ntg_amd"), "ntg_amd", ["-Wl,--no-undefined"])
    und = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    und = {l.split()[-1].split("@")[0] for l in und.splitlines() if l.split()}
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1].split("@")[0] for l in exported.splitlines() if len(l.split()) >= 3 and l.split()[1] in "TWiV"}
    for sym in ("ntg", "ntg_open", "ntg_close", "npsolCostFunction", "npsolConstraintFunction", "npsoloption", "SplineInterp", "DoubleMatrix"):
        assert sym in und and sym in exported, sym
