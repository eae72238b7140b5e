"""-m gpu: ntg_batch_extrema / Plan.extrema -- the minimum and maximum of every certifiable trajectory row over the horizon, by bisection.

References: the library's own envelope calls at nsub = 0 (the depth-0 identity, bit for bit), tests/extrema_oracle.py (the exact extrema in
rational arithmetic, and the definition's level algorithm in float64 for the inputs' margins, checked in tests/test_extrema_abi.py), and the
family's own callbacks through Plan.check (witness times and soundness), which also audits the sum-of-squares declarations.  Slack: twice
the row slack of the envelope calls, the header's rounding statement.  tol: one figure per case, max(1e-9 max |row bound or value|, 64
slack).  Shapes are small: 4 / 5 / 8 / 20 knot intervals (80 once, for the second pass over the intervals), batches 1 to 67."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import extrema_oracle as xo
from ntg_amd import api, configs as cf, family
from cert_common import NSAMP, cpu, full_list_problem
from gpu_common import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ext", "when", "status", "npieces", "viol", "where")


class Case:
    def __init__(self, name):
        self.c = c = xo.inputs(name)
        self.name, self.spec, self.nb = name, c.spec, c.x.shape[0]
        self.plan = api.Plan(c.spec, 0)
        self.flags = xo.flags(c.spec)
        self.table = xo.row_table(c.spec)
        self.nrow = c.spec.nltc + c.spec.nnltc
        if c.knots is not None:
            self.plan.set_grids(dev(c.knots), dev(c.bps), with_precond=False)
        self._all = None
        self._exact = None

    def args(self, sl=slice(None)):
        """x, lower, upper of problems sl on the device, their parameters set"""
        if self.c.prm is not None:
            self.plan.set_params(dev(self.c.prm[sl]))
        return dev(self.c.x[sl]), dev(self.c.lower[sl]), dev(self.c.upper[sl])

    def all(self):
        """the whole case at its tolerance, both sides, no bounds"""
        if self._all is None:
            xd, _, _ = self.args()
            self._all = cpu(self.plan.extrema(xd, self.c.tol))
        return self._all

    def exact(self):
        """[nexact, nrow, 4] (NaN for a row without a statement)"""
        if self._exact is None:
            c = self.c
            out = np.full((c.nexact, self.nrow, 4), np.nan)
            for b in range(c.nexact):
                ex = xo.exact_polygons(c.spec, c.x[b], None if c.prm is None else c.prm[b], None if c.knots is None else c.knots[b])
                for r in range(self.nrow):
                    if self.flags[r]:
                        out[b, r] = [float(v) for v in xo.exact_extrema(ex[r], c.sl[b, r] / 8)]
            self._exact = out
        return self._exact

    def times(self, b, n=NSAMP):
        """n times per knot interval of problem b, ends included"""
        kn = np.asarray(self.c.kn(b), dtype=np.float64)
        u = np.linspace(0.0, 1.0, n)
        t = kn[:-1, None] + (kn[1:] - kn[:-1])[:, None] * u[None, :]
        t[:, -1] = kn[1:]
        return np.clip(t, kn[0], kn[-1]).reshape(-1)

    def rows_at(self, t):
        """the family's rows through Plan.check: t [ntimes] (shared grid) or [nb, ntimes] (per-problem grids) -> [nb, nrow, ntimes]"""
        xd, lo, up = self.args()
        return cpu(self.plan.check(xd, lo, up, dev(np.ascontiguousarray(t)), want_rows=True))["rows"]


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=xo.CASES)
def case(request):
    return get_case(request.param)


# ---------------- 1. depth 0 is the envelope calls at nsub = 0 ----------------
def test_depth_zero_is_the_envelope_at_nsub_zero(case):
    xd, _, _ = case.args()
    got = cpu(case.plan.extrema(xd, case.c.tol, max_depth=0))
    assert case.plan.extrema_rows().tolist() == case.flags.tolist()
    sp = case.spec
    lo = np.full((case.nb, case.nrow), np.nan); hi = np.full_like(lo, np.nan)
    if sp.nltc:
        e = cpu(case.plan.envelope(xd, 0, want_entries=False, want_rows=True))
        lo[:, :sp.nltc], hi[:, :sp.nltc] = e["row_lo"].min(axis=2), e["row_hi"].max(axis=2)
    if sp.nnltc:
        e = cpu(case.plan.envelope_sos(xd, 0))
        lo[:, sp.nltc:], hi[:, sp.nltc:] = e["q_lo"].min(axis=2), e["q_hi"].max(axis=2)
    f = case.flags == 1
    assert np.array_equal(got["ext"][:, f, 0], lo[:, f]) and np.array_equal(got["ext"][:, f, 3], hi[:, f])
    assert np.isin(got["status"][:, f], (xo.OK, xo.DEPTH)).all() and (got["status"][:, f] == xo.DEPTH).any()
    l = np.array([sp.kninterv[o0] for _, o0, *_ in case.table])
    assert (got["npieces"][:, f] == l[f][None, :]).all()
    assert (got["status"][:, ~f] == xo.NONE).all() and (got["npieces"][:, ~f] == 0).all()


# ---------------- 2. enclosure of the exact extrema ----------------
def test_the_exact_extrema_are_enclosed_to_the_tolerance(case):
    got, c = case.all(), case.c
    f = case.flags == 1
    assert (got["status"][:, f] == xo.OK).all(), got["status"]
    ext, s = got["ext"][:, f], c.sl[:, f]
    assert (ext[..., 1] - ext[..., 0] <= c.tol + s).all() and (ext[..., 3] - ext[..., 2] <= c.tol + s).all()
    ex = case.exact()[:, f]
    e, s = ext[:c.nexact], s[:c.nexact]
    worst = float(max(((e[..., 0] - ex[..., 1]) / s).max(), ((ex[..., 0] - e[..., 1]) / s).max(), ((e[..., 2] - ex[..., 3]) / s).max(), ((ex[..., 2] - e[..., 3]) / s).max()))
    print(f"{case.name}: the exact extrema outside the enclosures by at most {worst:.3g} slack; tol {c.tol:.3g}; pieces per row {got['npieces'][:, f].mean():.1f}")
    assert worst <= 1.0
    assert (got["ext"][:, ~f] == np.array([-np.inf, np.inf, -np.inf, np.inf])).all() and np.isnan(got["when"][:, ~f]).all()


# ---------------- 3. the witness times ----------------
def test_the_rows_take_the_attained_values_at_the_witness_times(case):
    got, c = case.all(), case.c
    when = np.where(np.isnan(got["when"]), np.asarray(c.kn(0))[0], got["when"])   # (rows without a statement: any time of the horizon)
    if c.knots is None:
        rows = case.rows_at(when.reshape(-1)).reshape(case.nb, case.nrow, case.nb, case.nrow, 2)
        at = np.stack([rows[b, np.arange(case.nrow), b, np.arange(case.nrow)] for b in range(case.nb)])   # [nb, nrow, 2]
    else:
        rows = case.rows_at(when.reshape(case.nb, -1)).reshape(case.nb, case.nrow, case.nrow, 2)
        at = rows[:, np.arange(case.nrow), np.arange(case.nrow)]
    f = case.flags == 1
    err = np.abs(at[:, f] - got["ext"][:, f][..., 1:3]) / c.sl[:, f, None]
    print(f"{case.name}: the family's rows at the witness times differ from the attained values by at most {float(err.max()):.3g} slack")
    assert err.max() <= 2.0
    kn0 = np.array([np.asarray(c.kn(b))[[0, -1]] for b in range(case.nb)])
    assert (got["when"][:, f] >= kn0[:, None, None, 0]).all() and (got["when"][:, f] <= kn0[:, None, None, 1]).all()


# ---------------- 4. soundness against the library's own callbacks ----------------
def test_samples_stay_inside_the_enclosures(case):
    got, c = case.all(), case.c
    t = case.times(0) if c.knots is None else np.stack([case.times(b) for b in range(case.nb)])
    rows = case.rows_at(t)
    f = case.flags == 1
    s = c.sl[:, f, None]
    below, above = (got["ext"][:, f, 0, None] - rows[:, f]) / s, (rows[:, f] - got["ext"][:, f, 3, None]) / s
    worst = float(max(below.max(), above.max()))
    print(f"{case.name}: the family's rows outside the enclosures by at most {worst:.3g} slack")
    assert worst <= 1.0
    # ... and the attained values are no better than what the samples see
    assert (got["ext"][:, f, 1] <= rows[:, f].min(axis=2) + s[..., 0]).all() and (got["ext"][:, f, 2] >= rows[:, f].max(axis=2) - s[..., 0]).all()


# ---------------- 5. known answer ----------------
def test_known_answer():
    """x(t) = 8 t, y = y0: the row is 64 (t - 2.5)^2 + (y0 - 0.5)^2, closest to the obstacle at t = 2.5"""
    case = get_case("O20")
    spec, y0 = case.spec, 1.75
    gv = xo.greville(spec)
    x = np.concatenate([8.0 * gv, np.full(gv.size, y0)])[None, :]
    s = xo.slack(spec, x)[0, 0]
    lo, up = cf.obstacle_bounds(1, radius=3.0)
    tol = max(1e-9 * 400.0, 64 * s)
    got = cpu(case.plan.extrema(dev(x), tol, lower=dev(lo), upper=dev(up)))
    print("known answer:", got["ext"][0, 0], got["when"][0, 0], got["viol"][0], got["status"][0], got["npieces"][0], "slack", s, "tol", tol)
    want = (y0 - 0.5) ** 2
    assert got["status"][0, 0] == xo.OK
    assert got["ext"][0, 0, 0] - s <= want <= got["ext"][0, 0, 1] + s and got["ext"][0, 0, 1] - got["ext"][0, 0, 0] <= tol + s
    assert abs(got["when"][0, 0, 0] - 2.5) <= np.sqrt(tol / 64)
    assert abs(got["viol"][0, 0] - (9.0 - want)) <= s and abs(got["viol"][0, 1] - got["viol"][0, 0]) <= tol + s and got["viol"][0, 1] >= got["viol"][0, 0]
    assert got["where"][0].tolist() == [0, 0]
    assert abs(got["ext"][0, 0, 3] - (400.0 + want)) <= tol + s and got["when"][0, 0, 1] in (0.0, 5.0)   # the ends of the horizon are 20 away
    lo, up = cf.obstacle_bounds(1, radius=1.0)
    got = cpu(case.plan.extrema(dev(x), tol, lower=dev(lo), upper=dev(up)))
    assert got["viol"][0].tolist() == [0.0, 0.0] and got["where"][0].tolist() == [-1, -1]


# ---------------- 6. sides ----------------
def test_one_side_leaves_the_other_a_valid_enclosure(case):
    both, c = case.all(), case.c
    xd, _, _ = case.args()
    f = case.flags == 1
    ex = case.exact()[:, f]
    for sides in (1, 2):
        one = cpu(case.plan.extrema(xd, c.tol, sides=sides))
        assert (one["npieces"] <= both["npieces"]).all() and (one["status"][:, f] == xo.OK).all()
        e, s = one["ext"][:c.nexact, f], c.sl[:c.nexact, f]
        assert (e[..., 0] - s <= ex[..., 1]).all() and (ex[..., 0] <= e[..., 1] + s).all() and (e[..., 2] - s <= ex[..., 3]).all() and (ex[..., 2] <= e[..., 3] + s).all()
        k = 0 if sides == 1 else 2
        assert (one["ext"][:, f, k + 1] - one["ext"][:, f, k] <= c.tol + c.sl[:, f]).all()
    assert (one["npieces"][:, f] < both["npieces"][:, f]).any()


# ---------------- 7. early stops ----------------
def test_max_depth_stops_early_with_a_sound_enclosure(case):
    full, c = case.all(), case.c
    xd, _, _ = case.args()
    got = cpu(case.plan.extrema(xd, c.tol, max_depth=2))
    f = case.flags == 1
    need = full["npieces"][:, f] > got["npieces"][:, f]
    assert need.any() and (got["status"][:, f][need] == xo.DEPTH).all() and (got["status"][:, f][~need] == xo.OK).all()
    s = c.sl[:, f]
    assert (got["ext"][:, f, 0] <= full["ext"][:, f, 0] + s).all() and (got["ext"][:, f, 1] >= full["ext"][:, f, 1]).all()
    assert (got["ext"][:, f, 2] <= full["ext"][:, f, 2]).all() and (got["ext"][:, f, 3] >= full["ext"][:, f, 3] - s).all()


def test_more_intervals_than_lanes_and_a_full_list():
    """80 knot intervals: level 0 takes two passes.  y repeats one shape on every interval (control points -2 .. 3, -0.25 at the knots), so
    every interval's polygon reaches 0.75 or more below the smallest end value and all 80 pieces are open after level 0: more than the list holds.  (No FULL case with twice the capacity open was
    found on 20 intervals: rows that repeat one shape there keep at most 28 pieces open and end OK once the polygons are flat to rounding.)"""
    spec, x = full_list_problem()
    polys = xo.row_polygons(spec, x)
    ref = xo.level_oracle(polys[0][0], spec.knots[0], 0.0, sides=1)
    assert ref["status"] == xo.FULL and ref["max_open"] == 80 and ref["npieces"] == 80
    U = min(min(B[0], B[-1]) for B in polys[0][0])
    assert all(B.min() < U - 0.5 for B in polys[0][0])   # every decision of level 0 is far from the rounding
    p = api.Plan(spec, 0)
    lo = np.concatenate([np.zeros((1, 6)), [[-1.0]], np.zeros((1, 6)), [[9.0]]], axis=1); up = np.concatenate([np.zeros((1, 6)), [[1.0]], np.zeros((1, 6)), [[cf.INF_BOUND]]], axis=1)
    xd = dev(x)
    got = cpu(p.extrema(xd, 0.0, sides=1))
    assert got["status"][0, 0] == xo.FULL
    assert got["npieces"][0, 0] == 80
    zero = cpu(p.extrema(xd, 0.0, max_depth=0))
    e, q = cpu(p.envelope(xd, 0, want_entries=False, want_rows=True)), cpu(p.envelope_sos(xd, 0))
    assert zero["ext"][0, 0, 0] == e["row_lo"].min() and zero["ext"][0, 0, 3] == e["row_hi"].max()
    assert zero["ext"][0, 1, 0] == q["q_lo"].min() and zero["ext"][0, 1, 3] == q["q_hi"].max()
    s = xo.slack(spec, x)[0]
    assert got["ext"][0, 0, 0] == e["row_lo"].min() and abs(got["ext"][0, 0, 1] - ref["ext"][1]) <= s[0]
    t = np.linspace(0.0, 5.0, 80 * 8 + 1)
    rows = cpu(p.check(xd, dev(lo), dev(up), dev(t), want_rows=True))["rows"][0]
    deep = cpu(p.extrema(xd, 64 * s.max()))
    assert (deep["ext"][0, :, 0] - s <= rows.min(axis=1)).all() and (rows.max(axis=1) <= deep["ext"][0, :, 3] + s).all()
    assert deep["status"][0, 0] == xo.FULL and deep["status"][0, 1] in (xo.OK, xo.DEPTH)


# ---------------- 8. batch independence and repeatability ----------------
def test_a_problem_alone_and_the_same_call_twice():
    case = get_case("O4")
    xd, lo, up = case.args()
    a = cpu(case.plan.extrema(xd, case.c.tol, lower=lo, upper=up))
    b = cpu(case.plan.extrema(xd, case.c.tol, lower=lo, upper=up))
    one = cpu(case.plan.extrema(xd[5:6].contiguous(), case.c.tol, lower=lo[5:6].contiguous(), upper=up[5:6].contiguous()))
    assert set(a) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(one[k][0], a[k][5], equal_nan=True), k
    assert (a["viol"][:, 1] >= a["viol"][:, 0]).all() and (a["viol"][:, 0] > 0).any()


def test_violation_is_the_maximum_over_the_rows():
    case = get_case("K3")
    xd, lo, up = case.args()
    got = cpu(case.plan.extrema(xd, case.c.tol, lower=lo, upper=up))
    l, u = case.c.lower[:, 6:9], case.c.upper[:, 6:9]
    att = np.maximum(np.maximum(l - got["ext"][..., 1], got["ext"][..., 2] - u), 0.0)
    cer = np.maximum(np.maximum(l - got["ext"][..., 0], got["ext"][..., 3] - u), 0.0)
    assert np.array_equal(got["viol"][:, 0], att.max(axis=1)) and np.array_equal(got["viol"][:, 1], cer.max(axis=1))
    assert np.array_equal(got["where"][:, 0], np.where(att.max(axis=1) > 0, att.argmax(axis=1), -1))
    assert np.array_equal(got["where"][:, 1], np.where(cer.max(axis=1) > 0, cer.argmax(axis=1), -1))
    assert (got["viol"] > 0).any()


# ---------------- 9. per-problem grids: the G4 case of tests 1 to 4, on every problem's own knots ----------------
def test_grids_are_for_their_own_batch():
    case = get_case("G4")
    xd, _, _ = case.args()
    with pytest.raises(api.NtgError, match="-2"):
        case.plan.extrema(xd[:3].contiguous(), case.c.tol)
    own = cpu(api.Plan(dataclasses.replace(case.spec, knots=[case.c.knots[1].copy() for _ in range(2)], bps=case.c.bps[1].copy()), 0).extrema(xd[1:2].contiguous(), case.c.tol))
    s = case.c.sl[1]
    assert (np.abs(own["ext"][0] - case.all()["ext"][1]) <= case.c.tol + s[:, None]).all()


# ---------------- 10. flags ----------------
def test_flags_and_partial_certificates():
    case = get_case("T3")
    assert case.plan.extrema_rows().tolist() == [1, 1, 0]
    got = case.all()
    assert (got["status"][:, 2] == xo.NONE).all() and (got["status"][:, :2] == xo.OK).all()
    xd, lo, up = case.args()
    with pytest.raises(api.NtgError, match="-4") as e:
        case.plan.extrema(xd, case.c.tol, lower=lo, upper=up)
    assert "row 2" in str(e.value)
    tp = api.Plan(cf.config_T(), 0)   # the linear row names outputs of two basis classes, and so does nonlinear row 0
    assert tp.extrema_rows().tolist() == [0, 0, 0]
    with pytest.raises(api.NtgError, match="-4"):
        tp.extrema(dev(np.zeros((2, tp.spec.nC))), 1e-9)


def test_a_module_family_gets_its_linear_row_certified():
    case = get_case("T3")
    fam = api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "testfam_module.hip")))
    mp = api.Plan(dataclasses.replace(case.spec, family=fam), 0)
    assert mp.extrema_rows().tolist() == [1, 0, 0]
    xd, _, _ = case.args()
    got = cpu(mp.extrema(xd, case.c.tol))
    ref = case.all()
    for k in ("ext", "when", "status", "npieces"):
        assert np.array_equal(got[k][:, 0], ref[k][:, 0]), k
    assert (got["status"][:, 1:] == xo.NONE).all()


# ---------------- 11. NaN ----------------
def test_nan_marks_the_rows_that_name_it():
    case = get_case("K3")   # rows: y; x'; x' - y' + 0.5 y''
    xd, _, _ = case.args()
    x = case.c.x.copy()
    x[2, 1] = np.nan   # a coefficient of x on the first knot interval
    got, clean = cpu(case.plan.extrema(dev(x), case.c.tol)), case.all()
    for k in ("ext", "when", "status", "npieces"):
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
        assert np.array_equal(got[k][2, 0], clean[k][2, 0]), k   # y does not name it
    assert (got["status"][2, 1:] == xo.NAN).all() and np.isnan(got["ext"][2, 1:]).all() and np.isnan(got["when"][2, 1:]).all()


# ---------------- 12. refusals ----------------
def test_refusals():
    case = get_case("O4")
    xd, lo, up = case.args(slice(0, 2))
    L = api.lib()
    ptr = lambda t: None if t is None else t.data_ptr()
    ext = torch.empty((2, 1, 4), dtype=torch.float64, device="cuda:0")
    viol = torch.zeros((2, 2), dtype=torch.float64, device="cuda:0")

    def raw(batch=2, x=xd, tol=1e-9, depth=30, sides=3, lower=None, upper=None, e=ext, v=None):
        rc = L.ntg_batch_extrema(case.plan.h, batch, ptr(x), tol, depth, sides, ptr(lower), ptr(upper), ptr(e), None, None, None, ptr(v), None, None)
        return rc, L.ntg_last_error().decode()

    assert raw()[0] == 0
    for kw, word in ((dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"), (dict(depth=-1), "max_depth"), (dict(depth=31), "max_depth"),
                     (dict(sides=0), "sides"), (dict(sides=4), "sides"), (dict(x=None), "null"), (dict(e=None), "no output"), (dict(v=viol), "bounds")):
        rc, msg = raw(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    assert raw(batch=0, depth=31)[0] == -2 and raw(batch=0)[0] == 0 and raw(batch=0, x=None)[0] == 0   # the arguments before the empty batch
    assert raw(lower=lo, upper=up, v=viol)[0] == 0
    kp = api.Plan(cf._kincar_spec(1, 6, 3, 4, 21, 5.0, "kincar-l4"), 0)   # no trajectory rows at all
    assert kp.extrema_rows().shape == (0,)
    with pytest.raises(api.NtgError, match="-2") as e:
        kp.extrema(dev(np.zeros((2, kp.spec.nC))), 1e-9)
    assert "nltc + nnltc" in str(e.value)
    fp = api.Plan(cf.config_OF(3, ninterv=5), 0)        # the centres are parameters: not set yet
    with pytest.raises(api.NtgError, match="-2") as e:
        fp.extrema(dev(np.zeros((2, fp.spec.nC))), 1e-9)
    assert "ntg_plan_set_params" in str(e.value)
    fp.set_params(dev(np.zeros((3, 6))))
    with pytest.raises(api.NtgError, match="-2"):      # parameters for another batch
        fp.extrema(dev(np.zeros((2, fp.spec.nC))), 1e-9)
    mp = api.Plan(cf.config_E(ninterv=4, narms=2), 0)   # the manipulator's rows are sines and it has no linear row
    assert mp.extrema_rows().tolist() == [0, 0]
    with pytest.raises(api.NtgError, match="-4"):
        mp.extrema(dev(np.zeros((2, mp.spec.nC))), 1e-9)
    hp = api.Plan(dataclasses.replace(xo.rows_spec(), family=-1), 0)   # host-callback plans
    with pytest.raises(api.NtgError, match="-4"):
        hp.extrema(dev(np.zeros((2, hp.spec.nC))), 1e-9)
    # (nnltc > 8 cannot be reached: no family in the tree takes a plan with more than 8 nonlinear trajectory rows)
    bs = cf._kincar_spec(1, 6, 3, 300, 301, 5.0, "kincar-l300")   # 300 (36 + 2) + 1 doubles of tables and 4 (1806 + 768) of the waves: 170 KiB
    big = api.Plan(dataclasses.replace(bs, ltc=np.eye(1, 6, 3), lin_ineq=[0] * bs.nlic + [1] + [0] * bs.nlfc), 0)
    assert big.extrema_rows().tolist() == [1]
    with pytest.raises(api.NtgError, match="-4") as e:
        big.extrema(dev(np.zeros((2, big.spec.nC))), 1e-9)
    assert "LDS" in str(e.value)
