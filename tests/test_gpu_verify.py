"""-m gpu: ntg_batch_verify / Plan.verify -- a family's analytic derivatives and the plan's active-variable lists against central
differences at the breakpoints.

Reference: the CPU restatement tests/verify_oracle.py (the oracle's SplineInterp, the oracle's family functions or the host shims, the
definition of include/ntg_amd.h in float64), computed once per case.

Tolerances, measured against the restatement and not fixed here: N = the largest err and leak the restatement reports over all CLEAN slots of
a test's cases (test_verify_oracle.py asserts N <= 1e-8 and every planted defect >= 1e-3 on the CPU).
  clean slot    err <= 100 N and leak <= 100 N
  planted slot  |err_gpu - err_cpu| <= 100 N; where equals the restatement's in function and entry; at the GPU's breakpoint the restatement's
                table is within 100 N of its maximum (the breakpoint of a near-tie is decided by rounding)
Why 100: the device contracts multiply-adds and the shims are built with -ffp-contract=off, so the two sides' function values differ by a few
ulp of the intermediate magnitudes, and the quotient amplifies that by 1 / (2 h) ~ 6.6e4: noise of the size of N itself, not of a known
multiple of eps.  Every test prints N and the GPU maxima before it asserts."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

import verify_oracle as vo
from ntg_amd import api, configs as cf
from gpu_common import SPECS, dev
from test_gpu_grids import grids_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 128    # NTG_CHECK_NT: breakpoints of one tile
AMP = 0.3   # coefficients 0.3 * normal (test_verify_oracle.py: N <= 1e-8 with them)
KEYS = ("err", "where", "leak", "leak_where")


@pytest.fixture(scope="module")
def fams():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    src = {"unicycle": os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip"), "tracking": os.path.join(ROOT, "ntg_amd", "modules", "tracking.hip"),
           "miswired": os.path.join(ROOT, "tests", "modules", "miswired.hip")}
    return {m: api.load_family(family.build_module(s)) for m, s in src.items()}


def coefficients(spec, nb, seed=21):
    return AMP * np.random.default_rng(seed).normal(size=(nb, spec.nC))


def run(plan, x, want_leak=True):
    out = plan.verify(dev(x), want_leak=want_leak)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def debug_run(plan, x, cap):
    """ntg_debug_batch_verify: ntg_batch_verify with the scratch cap of the per-problem tables stated (forces several chunks)"""
    L = api.lib()
    L.ntg_debug_batch_verify.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_longlong]
    xd = dev(x); nb = xd.shape[0]
    err = torch.zeros((nb, 6), dtype=torch.float64, device="cuda:0"); leak = torch.zeros_like(err)
    wh = torch.full((nb, 6, 3), -7, dtype=torch.int32, device="cuda:0"); lw = torch.full_like(wh, -7)
    rc = L.ntg_debug_batch_verify(plan.h, nb, xd.data_ptr(), err.data_ptr(), wh.data_ptr(), leak.data_ptr(), lw.data_ptr(), None, cap)
    assert rc == 0, L.ntg_last_error().decode()
    torch.cuda.synchronize()
    return dict(err=err.cpu().numpy(), where=wh.cpu().numpy(), leak=leak.cpu().numpy(), leak_where=lw.cpu().numpy())


def bit_equal(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True) for k in a)


def check_clean(out, ref, spec, label, planted=()):
    """every slot outside `planted`: err and leak within 100 N; unused slots exactly 0 with no place.  Prints before it asserts."""
    N = vo.floor(ref, planted)
    clean = [s for s in range(6) if s not in planted]
    print(f"verify {label}: N {N:.3e} | gpu err {out['err'][:, clean].max():.3e} leak {out['leak'][:, clean].max():.3e} | per slot err "
          f"{np.array2string(out['err'].max(axis=0), precision=2)} leak {np.array2string(out['leak'].max(axis=0), precision=2)}")
    assert 0 < N <= 1e-8
    assert (out["err"][:, clean] <= 100 * N).all() and (out["leak"][:, clean] <= 100 * N).all()
    used = np.array([int(n) > 0 for n, _, _ in vo.slot_setup(spec)])
    assert (out["err"][:, ~used] == 0).all() and (out["leak"][:, ~used] == 0).all()
    assert (out["where"][:, ~used] == -1).all() and (out["leak_where"][:, ~used] == -1).all()
    for v, w in ((out["err"], out["where"]), (out["leak"], out["leak_where"])):   # a place exactly where the figure is not 0, inside the plan
        assert ((w[..., 0] >= 0) == (v != 0)).all()
        assert (w[..., 1] < spec.nbps).all() and (w[..., 2] < spec.nz).all()
        # the initial slots are audited at breakpoint 0 and the final slots at the last one, nowhere else
        assert (w[:, [0, 3], 1][v[:, [0, 3]] != 0] == 0).all() and (w[:, [2, 5], 1][v[:, [2, 5]] != 0] == spec.nbps - 1).all()
    # every slot the restatement sees something in ran on the device too (a slot that was skipped reads 0 and passes the bounds above)
    seen = np.nan_to_num(ref["err"], nan=1.0).max(axis=0) > 0
    assert (np.nan_to_num(out["err"], nan=1.0).max(axis=0)[seen] > 0).all()
    return N


def check_planted(out, ref, spec, N, label):
    P = spec.nbps
    for s, (kind, fn, entry) in vo.PLANTED.items():
        g, gw = (out["err"], out["where"]) if kind == "err" else (out["leak"], out["leak_where"])
        r, rw = (ref["err"], ref["where"]) if kind == "err" else (ref["leak"], ref["leak_where"])
        tabs = ref["e"] if kind == "err" else ref["l"]
        print(f"verify {label}: planted slot {s} {kind}: gpu {g[:, s]} cpu {r[:, s]} | gpu where {gw[:, s].tolist()} cpu where {rw[:, s].tolist()}")
        assert (r[:, s] >= 1e-3).all()
        assert (np.abs(g[:, s] - r[:, s]) <= 100 * N).all()
        assert (gw[:, s, 0] == fn).all() and (gw[:, s, 2] == entry).all() and (rw[:, s, 0] == fn).all() and (rw[:, s, 2] == entry).all()
        for b in range(g.shape[0]):
            bp = int(gw[b, s, 1])
            assert 0 <= bp < P
            assert abs(tabs[b][s][fn, bp, entry] - r[b, s]) <= 100 * N   # a near-tie's breakpoint is decided by rounding
        other = out["leak"] if kind == "err" else out["err"]
        assert (other[:, s] <= 100 * N).all()


# ---- 1. the built-in families are clean ----
BUILTIN = {"A": SPECS["A"], "K0": SPECS["K0"], "T": SPECS["T"], "O4": lambda: cf.config_O(ninterv=4), "D8": SPECS["D8"], "E8": SPECS["E8"],
           "M": SPECS["M"], "E8x3": lambda: cf.config_E(ninterv=8, narms=3)}   # E8x3: 9 outputs, the run-time-indexed path (NOUTMAX > 8)


@pytest.mark.parametrize("name", list(BUILTIN))
def test_builtin_families_are_clean(name):
    spec, cbs, _, _ = vo.builtin_case(BUILTIN[name]())
    x = coefficients(spec, 3)
    out = run(api.Plan(spec, 0), x)
    check_clean(out, vo.restate(spec, x, cbs), spec, name)


def test_unicycle_module_is_clean(fams):
    spec, cbs, _, _ = vo.unicycle_case(fams["unicycle"])
    x = coefficients(spec, 3)
    out = run(api.Plan(spec, 0), x)
    check_clean(out, vo.restate(spec, x, cbs), spec, "unicycle")


# ---- 2. tile edges, workgroups that walk over several problems, the tie-break ----
@pytest.mark.parametrize("nbps", [64, 65, 130])
def test_tile_edges(nbps):
    """130: two tiles, the second with two live lanes; 64 / 65: a wave boundary.  testfam: all six slots, so the final slots sit in the
    last tile's last live lane"""
    spec, cbs, _, _ = vo.builtin_case(cf.config_T(nbps=nbps))
    x = coefficients(spec, 3, seed=nbps)
    out = run(api.Plan(spec, 0), x)
    check_clean(out, vo.restate(spec, x, cbs), spec, f"T nbps {nbps}")


def test_a_workgroup_walks_over_several_problems():
    """the launcher's rule (time_tile_walk): gridDim.y = min(batch, max(1, ceil(8 ncu / ntiles))).  Enough breakpoint tiles that 64 problems
    are more than the groups, so that the first groups' workgroups take two problems; the problems repeat 2 coefficient rows in a random
    order (a wrong problem index shows in half of the cases), and every problem must be bit-equal to its row's result alone"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ntiles = (8 * ncu + 59) // 60
    nbps = ntiles * NT - 28
    groups = max(1, (8 * ncu + ntiles - 1) // ntiles)
    batch = 64
    assert groups < batch, (ncu, ntiles, groups)
    spec = cf._kincar_spec(1, 6, 3, 20, nbps, 5.0, "kincar-many-bps")
    cbs = vo.builtin_callbacks(spec)
    x2 = coefficients(spec, 2, seed=4)
    idx = np.random.default_rng(9).integers(0, 2, batch)
    idx[:2] = (0, 1); idx[-2:] = (1, 0)
    p = api.Plan(spec, 0)
    out = run(p, x2[idx])
    print(f"ncu {ncu} tiles {ntiles} nbps {nbps} groups {groups} batch {batch}")
    check_clean(out, vo.restate(spec, x2, cbs), spec, "walk")
    alone = run(p, x2)
    assert bit_equal(out, alone, rows_b=idx)


def test_tie_break(fams):
    """Two breakpoints with bit-identical flags: breakpoints on a dyadic grid (spacing 1/8, knots 1/2 apart, so t - knot is the same
    number in every interval) and coefficients that repeat from interval to interval (period order - mult = the coefficient offset
    between neighbouring intervals).  The planted sign error of the running cost then has the same value at breakpoint i and i + 4 of
    the interior intervals: the smaller index must be reported."""
    spec, cbs, _, _ = vo.miswired_case(fams["miswired"])
    spec = dataclasses.replace(spec, bps=cf.linspace_c(0.0, 4.0, 33))
    per = spec.order[0] - spec.mult[0]
    rng = np.random.default_rng(5)   # (a seed whose maxima lie in the interior intervals; the premise is asserted below)
    x = np.stack([np.concatenate([np.tile(AMP * rng.normal(size=per), spec.ncoef[o] // per) for o in range(spec.nout)]) for _ in range(2)])
    assert x.shape == (2, spec.nC)
    ref = vo.restate(spec, x, cbs)
    out = run(api.Plan(spec, 0), x)
    for b in range(2):
        tab = ref["e"][b][1][0, :, 2]   # slot ucf, function 0, entry (output 0, deriv 2): the planted one
        ties = np.flatnonzero(tab == tab.max())
        print(f"tie-break problem {b}: cpu max {tab.max():.6e} at breakpoints {ties.tolist()} | gpu {out['err'][b, 1]:.6e} where {out['where'][b, 1].tolist()}")
        assert ties.size >= 2 and tab.max() >= 1e-3   # the premise: the maximum is attained at several breakpoints, bit for bit
        assert out["where"][b, 1].tolist() == [0, int(ties[0]), 2] == ref["where"][b, 1].tolist()


# ---- 3. the planted defects ----
def test_planted_defects_are_found_where_they_were_planted(fams):
    spec, cbs, _, _ = vo.miswired_case(fams["miswired"])
    x = coefficients(spec, 3)
    ref = vo.restate(spec, x, cbs)
    out = run(api.Plan(spec, 0), x)
    N = check_clean(out, ref, spec, "miswired", planted=vo.PLANTED)
    check_planted(out, ref, spec, N, "miswired")


# ---- 4. parameters: per breakpoint (tracking module), per row function and problem (obstacle field) ----
def test_tracking_module_with_per_breakpoint_parameters(fams):
    nb = 3
    spec, cbs, setp, prm = vo.tracking_case(fams["tracking"], nb)
    p = api.Plan(spec, 0)
    x = coefficients(spec, nb)
    with pytest.raises(api.NtgError, match="-2"):   # NTG_E_BADARG: parameters needed but not set
        p.verify(dev(x))
    p.set_params(dev(prm))
    out = run(p, x)
    check_clean(out, vo.restate(spec, x, cbs, set_problem=setp), spec, "tracking")


def test_obstacle_field_with_per_problem_centres():
    nb = 4
    spec, cbs, setp, prm = vo.obstacle_field_case(nb, 3)
    p = api.Plan(spec, 0)
    p.set_params(dev(prm))
    x = coefficients(spec, nb)
    out = run(p, x)
    check_clean(out, vo.restate(spec, x, cbs, set_problem=setp), spec, "OF")
    # the figures of problem b do not change when another problem's parameters do
    prm2 = prm.copy(); prm2[0] += 1.5
    p.set_params(dev(prm2))
    out2 = run(p, x)
    assert bit_equal(out, out2, rows_a=slice(1, None), rows_b=slice(1, None))
    assert not np.array_equal(out["err"][0], out2["err"][0])   # ... and problem 0's do (rounding noise of other numbers)


# ---- 5. per-problem grids ----
def one_class_T():
    """testfam with every output on the same spline (per-problem grids need one basis class)"""
    s = cf.config_T()
    l, k = s.kninterv[0], s.order[0]
    return dataclasses.replace(s, kninterv=[l] * s.nout, order=[k] * s.nout, knots=[np.asarray(s.knots[0]).copy() for _ in range(s.nout)])


@pytest.mark.parametrize("name", ["T", "O"])
def test_per_problem_grids(name):
    spec = one_class_T() if name == "T" else cf.config_O(ninterv=4)
    nb = 4
    knots, bps = grids_for(spec, nb, warp=0.2)
    p = api.Plan(spec, 0)
    x = coefficients(spec, nb)
    shared = run(p, x)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    out = run(p, x)
    ref = vo.restate(spec, x, vo.builtin_callbacks(spec), knots=knots, bps=bps)   # every problem on its own knots and breakpoints
    check_clean(out, ref, spec, name + " on per-problem grids")
    assert not bit_equal(out, shared)            # the grids do differ
    chunks = debug_run(p, x, 1)                  # a cap of one byte: one problem per chunk, 4 chunks
    assert bit_equal(out, chunks)
    with pytest.raises(api.NtgError, match="-2"):   # the grids are for exactly this batch
        p.verify(dev(x[:2]))
    p.clear_grids()
    assert bit_equal(run(p, x), shared)


# ---- 6. determinism and independence ----
def test_results_are_bit_identical():
    spec = cf.config_T(nbps=130)
    p = api.Plan(spec, 0)
    x = coefficients(spec, 37, seed=8)
    a, b = run(p, x), run(p, x)
    assert bit_equal(a, b)                                         # call to call
    for i in (0, 17, 36):
        assert bit_equal(run(p, x[i:i + 1]), a, rows_b=slice(i, i + 1))   # problem i alone


# ---- 7. argument errors and edge cases ----
def test_tile_tables_beyond_the_lds_are_refused():
    """NTG_E_UNSUPPORTED for a plan whose tile tables exceed the LDS: six kincar outputs of order 10 on six different knot sequences are six
    basis classes of k d = 30 table rows each, 180 rows of 129 doubles = 185760 bytes for one tile, above 160 KiB.  Nothing is written.
    (The third NTG_E_UNSUPPORTED of the header, a plan shape the family has no instance for, cannot be reached through a device plan:
    ntg_plan_create refuses a maxderiv other than the family's and more than NTG_MAX_OUT = 16 outputs, every family but the manipulator
    has an NTG_MAX_NZ instance, and the manipulator's 48 entries hold its largest plan, 15 outputs of maxderiv 3.  It guards the
    launchers against a descriptor that does not match its kernels, and no test builds one.)"""
    spec = cf._kincar_spec(3, 10, 3, 4, 21, 5.0, "kincar-six-classes-k10")
    nints = [4, 5, 6, 7, 8, 9]
    spec = dataclasses.replace(spec, kninterv=nints, knots=[cf.linspace_c(0.0, 5.0, l + 1) for l in nints])
    assert sum(k * d for k, d in zip(spec.order, spec.maxderiv)) * (NT + 1) * 8 > 160 * 1024
    p = api.Plan(spec, 0)
    nb = 2
    x = dev(coefficients(spec, nb))
    L = api.lib()
    err = torch.full((nb, 6), 7.0, dtype=torch.float64, device="cuda:0"); leak = torch.full_like(err, 7.0)
    wh = torch.full((nb, 6, 3), -7, dtype=torch.int32, device="cuda:0"); lw = torch.full_like(wh, -7)
    assert L.ntg_batch_verify(p.h, nb, x.data_ptr(), err.data_ptr(), wh.data_ptr(), leak.data_ptr(), lw.data_ptr(), None) == -4
    assert "exceed 160 KiB" in L.ntg_last_error().decode()
    torch.cuda.synchronize()
    assert (err.cpu().numpy() == 7.0).all() and (leak.cpu().numpy() == 7.0).all()
    assert (wh.cpu().numpy() == -7).all() and (lw.cpu().numpy() == -7).all()


def test_refusals_and_degenerate_calls():
    spec, nb = cf.config_T(), 4
    p = api.Plan(spec, 0)
    x = dev(coefficients(spec, nb))
    L = api.lib()
    err = torch.full((nb, 6), 7.0, dtype=torch.float64, device="cuda:0")
    X, E = x.data_ptr(), err.data_ptr()
    assert L.ntg_batch_verify(p.h, 0, X, E, None, None, None, None) == 0 and L.ntg_batch_verify(p.h, -3, X, E, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (err.cpu().numpy() == 7.0).all()                                        # nothing ran
    assert L.ntg_batch_verify(None, nb, X, E, None, None, None, None) == -2        # null plan
    assert L.ntg_batch_verify(p.h, nb, None, E, None, None, None, None) == -2      # null d_x
    assert L.ntg_batch_verify(p.h, nb, X, None, None, None, None, None) == -2      # all outputs null
    assert "no output" in L.ntg_last_error().decode()
    host = api.Plan(dataclasses.replace(cf.config_B(), family=-1), 0)              # NTG_FAM_HOST
    with pytest.raises(api.NtgError, match="-4") as e:
        host.verify(dev(np.ones((nb, host.spec.nC))))
    assert "host-callback plans" in str(e.value)
    of = api.Plan(cf.config_OF(3, ninterv=4), 0)                                   # parameters: not set, then set for another batch
    prm, _, _ = cf.obstacle_field_problems(nb, 3)
    xf = dev(np.ones((nb, of.spec.nC)))
    with pytest.raises(api.NtgError, match="-2"):
        of.verify(xf)
    of.set_params(dev(prm))
    assert of.verify(xf)["err"].shape == (nb, 6)
    with pytest.raises(api.NtgError, match="-2"):
        of.verify(xf[:2].contiguous())
    # each output pointer alone works, and gives what the full call gives
    full = run(p, x.cpu().numpy())
    bufs = dict(err=torch.zeros((nb, 6), dtype=torch.float64, device="cuda:0"), where=torch.zeros((nb, 6, 3), dtype=torch.int32, device="cuda:0"),
                leak=torch.zeros((nb, 6), dtype=torch.float64, device="cuda:0"), leak_where=torch.zeros((nb, 6, 3), dtype=torch.int32, device="cuda:0"))
    for i, k in enumerate(KEYS):
        args = [None] * 4
        args[i] = bufs[k].data_ptr()
        assert L.ntg_batch_verify(p.h, nb, X, *args, None) == 0, L.ntg_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(bufs[k].cpu().numpy(), full[k])
    assert set(p.verify(x, want_leak=False)) == {"err", "where"}


def test_a_nan_stays_in_the_maximum():
    """a NaN coefficient: NaN err in the slots that see it (a middle coefficient of output 0: the trajectory slots; the initial and final
    points lie outside its support), the other problems untouched"""
    spec = cf.config_T()
    p = api.Plan(spec, 0)
    x = coefficients(spec, 3)
    clean = run(p, x)
    xn = x.copy(); xn[1, spec.ncoef[0] // 2] = np.nan
    out = run(p, xn)
    print("nan: err", out["err"][1], "where", out["where"][1].tolist())
    assert np.isnan(out["err"][1, 1]) and np.isnan(out["err"][1, 4])        # ucf, nltcf
    assert (out["where"][1, [1, 4]] >= 0).all()                             # ... with the place of the first NaN
    assert np.array_equal(out["err"][1, [0, 2, 3, 5]], clean["err"][1, [0, 2, 3, 5]])   # the slots at the ends do not see it
    assert bit_equal(out, clean, rows_a=[0, 2], rows_b=[0, 2])
