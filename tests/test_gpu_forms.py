"""-m gpu: ntg_batch_forms / Plan.forms -- certified extrema over the horizon of quadratic forms of the flag declared at the call.

References: tests/forms_oracle.py (the definition in float64; that it encloses the exact extrema, and the margins of its decisions to their
limits, are checked in tests/test_forms_oracle.py), the library's own ntg_batch_extrema where a form is one of its rows (bit for bit for
sums of squares, within slack for linear rows), Plan.interp (witness times and soundness) and ntg_batch_kincar_reverse (the steering
certificate).  Slack: the header's rounding statement, 2^-39 sum_t |w_t| S_u S_v.  tol: one figure per case, max(1e-9 max |polygon point|,
64 slack).  Shapes are small: 4 / 8 / 20 knot intervals (80 once, for the second pass over the intervals), 2 to 24 problems."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import extrema_oracle as xo
import forms_oracle as fo
import separation_oracle as po
from cert_common import cpu, field_x, piece_times, scaled_grids
from gpu_common import dev
from ntg_amd import api, configs as cf, forms as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ext", "when", "status", "npieces")


@pytest.fixture(scope="module")
def module_family():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))


class Case:
    def __init__(self, name, family=None):
        self.c = c = fo.inputs(name)
        self.name, self.nb, self.nform = name, c.x.shape[0], len(c.forms)
        self.spec = c.spec if family is None else dataclasses.replace(c.spec, family=family)
        self.plan = api.Plan(self.spec, 0)
        if c.knots is not None:
            self.plan.set_grids(dev(c.knots), dev(c.bps))
        self.xd, self.fd = dev(c.x), None if c.fprm is None else dev(c.fprm)
        # bounds that cut through the forms' ranges: the medians over the batch of the attained minimum and maximum; the last form has none
        ext = np.array([[r["ext"] for r in row] for row in c.levels()])
        self.lo = np.tile(np.median(ext[:, :, 1], axis=0), (self.nb, 1)); self.up = np.tile(np.median(ext[:, :, 2], axis=0), (self.nb, 1))
        self.lo[:, -1], self.up[:, -1] = -cf.INF_BOUND, cf.INF_BOUND
        self._runs = {}

    def run(self, tol=None, max_depth=30, bounds=True):
        key = (tol, max_depth, bounds)
        if key not in self._runs:
            kw = dict(lower=dev(self.lo), upper=dev(self.up)) if bounds else {}
            self._runs[key] = cpu(self.plan.forms(self.xd, self.c.forms, self.c.tol if tol is None else tol, max_depth, fprm=self.fd, **kw))
        return self._runs[key]


_cases = {}


def get_case(name, family=None):
    if name not in _cases:
        _cases[name] = Case(name, family)
    return _cases[name]


@pytest.fixture(scope="module", params=fo.CASES)
def case(request):
    return get_case(request.param, request.getfixturevalue("module_family") if request.param == "MOD" else None)


def same_as_oracle(got, ref, sl, label, knots=None):
    """status and npieces equal; ext and when within the slack.  ref [nb][nform] of level_oracle's dicts.  knots: the case repeats one shape
    on every knot interval (L80), so its smallest and largest end values are ties between the knots, which rounding decides: the witness
    times are then only asked to be knots"""
    assert got["status"].tolist() == [[r["status"] for r in row] for row in ref], label
    assert got["npieces"].tolist() == [[r["npieces"] for r in row] for row in ref], label
    rext, rwhen = np.array([[r["ext"] for r in row] for row in ref]), np.array([[r["when"] for r in row] for row in ref])
    err = float((np.abs(got["ext"] - rext) / sl[:, :, None]).max())
    if knots is None:
        err = max(err, float((np.abs(got["when"] - rwhen) / sl[:, :, None]).max()))
    else:
        assert np.isin(got["when"], knots).all() and np.isin(rwhen, knots).all(), label
    print(f"{label}: ext and when differ from the oracle's by at most {err:.3g} slack; {got['npieces'].mean():.1f} polygons per form")
    assert err <= 1.0, label
    return rext


def oracle_violation(rext, lo, up):
    vw = [fo.violation(rext[b], lo[b], up[b]) for b in range(len(rext))]
    return np.array([v for v, _ in vw]), np.array([w for _, w in vw])


# ---------------- 1. against the oracle (6. the violation figures) ----------------
def test_against_the_oracle(case):
    c = case.c
    got = case.run()
    assert set(got) == set(KEYS + ("viol", "where"))
    rext = same_as_oracle(got, c.levels(), c.sl, case.name, np.asarray(c.spec.knots[0]) if case.name == "L80" else None)
    assert (got["status"] == c.expect).all()
    if c.expect == fo.OK:
        assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= c.tol).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= c.tol).all()
    rv, rw = oracle_violation(rext, case.lo, case.up)
    err = float((np.abs(got["viol"] - rv) / c.sl.max(axis=1)[:, None]).max())
    print(f"{case.name}: viol differs from the oracle's by at most {err:.3g} slack; attained > 0 in {(got['viol'][:, 0] > 0).sum()} of {case.nb} problems")
    assert err <= 1.0 and np.array_equal(got["where"], rw)
    assert (got["viol"][:, 1] >= got["viol"][:, 0]).all()
    assert (got["where"] != case.nform - 1).all()            # a form with both bounds absent contributes nothing
    if case.nb >= 4:
        assert 0 < (got["viol"][:, 0] > 0).sum()             # the bounds do cut through the forms' ranges
    without = case.run(bounds=False)
    assert set(without) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(got[k], without[k]), k


# ---------------- 2. bit for bit against code that exists today ----------------
@pytest.mark.parametrize("which", ["OF4", "D8", "OF4-grids"])
def test_bit_for_bit_the_rows_of_extrema(which):
    if which == "D8":    # speed^2 = x'^2 + y'^2 + z'^2 is nonlinear row 1 of the quadrotor plan
        d8 = xo.inputs("D8")
        spec = d8.spec
        plan, x, prm, knots = api.Plan(spec, 0), d8.x, None, None
        form, row, tol = fm.speed2(spec, (0, 1, 2)), spec.nltc + 1, d8.tol
    else:                # (x - cx)^2 + (y - cy)^2 with the centre in the family's parameters, and in fprm
        spec = cf.config_OF(1, ninterv=4)
        nb = 12
        prm, lo, _ = cf.obstacle_field_problems(nb, 1)
        plan, x, knots = api.Plan(spec, 0), field_x(spec, lo, 32), None
        plan.set_params(dev(prm))
        if which == "OF4-grids":
            scales = np.linspace(0.5, 2.0, nb)
            knots, bps = scaled_grids(spec, scales)
            plan.set_grids(dev(knots), dev(bps))
        form, row, tol = fm.square(fm.entry(spec, 0, 0), param=0) + fm.square(fm.entry(spec, 1, 0), param=1), spec.nltc, 1e-6
    ref = cpu(plan.extrema(dev(x), tol))
    got = cpu(plan.forms(dev(x), [form], tol, fprm=None if prm is None else dev(prm)))
    assert (ref["status"][:, row] == xo.OK).all() and ref["npieces"][:, row].max() > spec.kninterv[0]
    for k in KEYS:
        assert np.array_equal(got[k][:, 0], ref[k][:, row]), k


# ---------------- 3. linear forms against extrema's linear rows ----------------
def test_linear_forms_against_the_linear_rows_of_extrema():
    s = cf._kincar_spec(1, 6, 3, 4, 21, 5.0, "kincar-2out-k6-l4")
    ltc = np.zeros((3, s.nz))
    ltc[0, 3] = 1.0; ltc[1, 1] = 1.0; ltc[2, 1] = 1.0; ltc[2, 4] = -1.0; ltc[2, 5] = 0.5   # cert_common.rows_spec's rows: y; x'; x' - y' + 0.5 y''
    spec = dataclasses.replace(s, ltc=ltc, lin_ineq=[0] * s.nlic + [1] * 3 + [0] * s.nlfc)
    plan = api.Plan(spec, 0)
    x = np.random.default_rng(33).standard_normal((7, spec.nC))
    forms = [fm.linear(3, 1.0), fm.linear(1, 1.0), fm.linear(1, 1.0) + fm.linear(4, -1.0) + fm.linear(5, 0.5)]
    sl = xo.slack(spec, x)           # extrema's slack of a linear row (the forms' own statement for the same row is four times that)
    tol = 64.0 * float(sl.max())
    ref, got = cpu(plan.extrema(dev(x), tol)), cpu(plan.forms(dev(x), forms, tol))
    err = float((np.abs(got["ext"] - ref["ext"]) / sl[:, :, None]).max())
    print(f"linear forms differ from extrema's linear rows by at most {err:.3g} slack")
    assert err <= 2.0
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == xo.OK).all()


# ---------------- 4. soundness against samples, and the witness times ----------------
@pytest.mark.parametrize("name", ["K4", "D8", "T4", "PP"])
def test_samples_lie_inside_and_the_witness_times_attain(name):
    case = get_case(name)
    c, got = case.c, case.run()
    vals = np.empty((case.nb, 0, case.nform))
    per = c.knots is not None
    for f in range(case.nform):
        ends = np.stack([np.asarray(c.kn(b, f), dtype=np.float64) for b in range(case.nb if per else 1)])
        t = np.stack([piece_times(e).reshape(-1) for e in ends])
        t = np.concatenate([t, got["when"][:, f, :] if per else got["when"][:, f, :].reshape(1, -1)], axis=1)
        z = cpu({"z": case.plan.interp(case.xd, dev(t if per else t[0]))})["z"]
        v = fo.values(case.spec, z, c.forms, c.fprm)[:, :, f]
        sl = c.sl[:, f][:, None]
        ns = t.shape[1] - (2 if per else 2 * case.nb)
        assert (v[:, :ns] >= got["ext"][:, f, 0][:, None] - sl).all() and (v[:, :ns] <= got["ext"][:, f, 3][:, None] + sl).all(), (name, f)
        w = v[:, ns:] if per else np.stack([v[b, ns + 2 * b:ns + 2 * b + 2] for b in range(case.nb)])
        err = float((np.abs(w - got["ext"][:, f, 1:3]) / sl).max())
        print(f"{name} form {f}: the values at the witness times differ from min_hi / max_lo by at most {err:.3g} slack")
        assert err <= 1.0, (name, f)


# ---------------- 5. the steering certificate, end to end ----------------
def test_steering_certificate_of_the_kinematic_car():
    case = get_case("K20")
    c, got = case.c, case.run()
    L = 3.0
    bound = fm.steering_bound(got["ext"], L)
    ref = fm.steering_bound(np.array([[r["ext"] for r in row] for row in c.levels()]), L)
    moving = got["ext"][:, 0, 0] > 0.0
    assert 2 * moving.sum() >= case.nb and np.array_equal(moving, np.isfinite(ref)) and np.isinf(bound[~moving]).all()
    kn = np.asarray(c.spec.knots[0])
    u = np.linspace(0.0, 1.0, 33)
    t = np.unique(np.clip((kn[:-1, None] + np.diff(kn)[:, None] * u[None, :]).reshape(-1), kn[0], kn[-1]))
    z = case.plan.interp(case.xd, dev(t))
    state = cpu({"s": case.plan.kincar_reverse(z, wheelbase=L)})["s"]     # [nb, nt, 1, 5] = x, y, theta, v, delta
    tan = np.abs(np.tan(state[:, :, 0, 4])).max(axis=1)
    print("largest sampled |tan delta| / certified bound:", np.round(tan[moving] / bound[moving], 4))
    assert (tan[moving] <= bound[moving] * (1.0 + 1e-9)).all()


# ---------------- 7. NaN ----------------
def test_nan_marks_the_forms_that_name_it():
    case = get_case("K4")   # all six of its forms name y: two forms of x alone join them
    c, clean = case.c, case.run(bounds=False)
    x = c.x.copy()
    x[5, c.spec.ncoef[0] + 1] = np.nan   # a coefficient of y on the first knot interval of problem 5
    names_y = [any(fo.so.entry_of(c.spec, v)[0] == 1 for t in form for v in (t.u, t.v) if v >= 0) for form in c.forms]
    forms = c.forms + [fm.square(fm.entry(c.spec, 0, 1)), fm.linear(fm.entry(c.spec, 0, 0), 2.0)]   # two forms of x alone
    got = cpu(case.plan.forms(dev(x), forms, c.tol, fprm=case.fd))
    ref = cpu(case.plan.forms(case.xd, forms, c.tol, fprm=case.fd))
    named = np.array(names_y + [False, False])
    assert named.sum() == 6 and np.array_equal(ref["ext"][:, :6], clean["ext"])
    for k in KEYS:
        assert np.array_equal(np.delete(got[k], 5, axis=0), np.delete(ref[k], 5, axis=0)), k
        assert np.array_equal(got[k][5, ~named], ref[k][5, ~named]), k
    assert (got["status"][5, named] == fo.NAN).all() and np.isnan(got["ext"][5, named]).all() and np.isnan(got["when"][5, named]).all()


# ---------------- 8. statuses ----------------
def test_depth_and_full_agree_with_the_oracle():
    case = get_case("K4")
    c = case.c
    got, ref = case.run(tol=0.0, max_depth=3, bounds=False), c.levels(0.0, 3)
    same_as_oracle(got, ref, c.sl, "K4, tol 0, max_depth 3")
    assert (got["status"] == fo.DEPTH).sum() >= case.nb and set(np.unique(got["status"])) <= {fo.OK, fo.DEPTH}
    full = get_case("L80")
    got, ref = full.run(tol=0.0, bounds=False), full.c.levels(0.0)
    same_as_oracle(got, ref, full.c.sl, "L80, tol 0", np.asarray(full.c.spec.knots[0]))
    assert (got["status"] == fo.FULL).all() and (got["npieces"] == 80).all()


# ---------------- 9. batch independence and repeatability ----------------
def test_batch_independence_repeatability_and_order_of_forms():
    case = get_case("K4")
    c, all24 = case.c, case.run(bounds=False)
    again = cpu(case.plan.forms(case.xd, c.forms, c.tol, fprm=case.fd))
    one = cpu(case.plan.forms(dev(c.x[19:20]), c.forms, c.tol, fprm=dev(c.fprm[19:20])))
    idx = [3, 19, 7, 0, 11]
    five = cpu(case.plan.forms(dev(c.x[idx]), c.forms, c.tol, fprm=dev(c.fprm[idx])))
    perm = [4, 2, 5, 0, 3, 1]
    shuffled = cpu(case.plan.forms(case.xd, [c.forms[i] for i in perm], c.tol, fprm=case.fd))
    for k in KEYS:
        assert np.array_equal(all24[k], again[k]), k
        assert np.array_equal(one[k][0], all24[k][19]) and np.array_equal(five[k][1], all24[k][19]), k
        assert np.array_equal(shuffled[k], all24[k][:, perm]), k


# ---------------- 10. refusals that need a plan ----------------
def test_refusals():
    case = get_case("K4")
    c = case.c
    L = api.lib()
    ptr = lambda t: None if t is None else t.data_ptr()
    ext = torch.empty((2, 8, 4), dtype=torch.float64, device="cuda:0")
    viol = torch.zeros((2, 2), dtype=torch.float64, device="cuda:0")
    x2, f2 = dev(c.x[:2]), dev(c.fprm[:2])

    def raw(plan=case.plan, forms=None, batch=2, x=x2, nfp=3, fprm=f2, tol=1e-6, depth=30, sides=3, lo=None, up=None, e=ext, v=None):
        forms = c.forms[:2] if forms is None else forms
        nt = (api.C.c_int * len(forms))(*[len(f) for f in forms])
        flat = [api.FormTerm(*t) for f in forms for t in f]
        rc = L.ntg_batch_forms(plan.h, batch, ptr(x), len(forms), nt, (api.FormTerm * max(len(flat), 1))(*flat), nfp, ptr(fprm), tol, depth, sides, ptr(lo), ptr(up),
                               ptr(e), None, None, None, ptr(v), None, None)
        return rc, L.ntg_last_error().decode()

    assert raw()[0] == 0
    t0 = c.forms[0][0]
    for kw, word in ((dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(depth=31), "max_depth"), (dict(sides=0), "sides"), (dict(x=None), "null"),
                     (dict(e=None), "no output"), (dict(v=viol), "bounds"), (dict(nfp=-1), "nfp"), (dict(forms=[c.forms[0]] * 9), "nform"),
                     (dict(forms=[c.forms[0], []]), "form 1 has 0 terms"), (dict(forms=[c.forms[0], c.forms[1] * 5]), "form 1 has 10 terms"),
                     (dict(forms=[c.forms[0], [t0._replace(u=6)]]), "form 1, term 0: u = 6"), (dict(forms=[[t0, t0._replace(v=-2)]]), "form 0, term 1: v = -2"),
                     (dict(forms=[[t0._replace(pu=3)]]), "form 0, term 0: pu and pv"), (dict(forms=[c.forms[3]], fprm=None), "form 0, term 1 names a parameter"),
                     (dict(forms=[[t0._replace(w=float("inf"))]]), "form 0, term 0: w, su and sv"), (dict(forms=[[t0._replace(sv=float("nan"))]]), "finite")):
        rc, msg = raw(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    assert raw(forms=[[fm.linear(0, 1.0)[0]._replace(sv=float("nan"), pv=7)]])[0] == 0   # sv and pv of a linear term are ignored
    assert raw(batch=0, depth=31)[0] == -2 and raw(batch=0)[0] == 0 and raw(forms=[])[0] == 0   # the arguments before the empty batch and the empty declaration
    lo = dev(np.zeros((2, 2)))
    assert raw(lo=lo, up=lo, v=viol)[0] == 0 and raw(lo=lo, v=viol)[0] == -2
    t4 = get_case("T4")
    with pytest.raises(api.NtgError, match="-4") as e:      # a form across the two basis classes
        t4.plan.forms(t4.xd, [t4.c.forms[0], fo.cross_class_form(t4.spec)], 1e-6)
    assert "form 1 names outputs 0 and 2 of different basis classes" in str(e.value)
    pp = get_case("PP")
    with pytest.raises(api.NtgError, match="-2") as e:      # a batch other than the grids'
        pp.plan.forms(dev(pp.c.x[:5]), pp.c.forms, 1e-6)
    assert "per-problem grids" in str(e.value)
    hp = api.Plan(dataclasses.replace(xo.rows_spec(), family=-1), 0)   # host-callback plans
    with pytest.raises(api.NtgError, match="-4") as e:
        hp.forms(dev(np.zeros((2, hp.spec.nC))), [fm.square(0)], 1e-6)
    assert "host-callback" in str(e.value)
    big = api.Plan(cf._kincar_spec(1, 6, 3, 300, 301, 5.0, "kincar-l300"), 0)   # 300 (36 + 2) + 1 doubles of tables, 3025 weights and 4 (1806 + 768) of the waves: 190 KiB
    with pytest.raises(api.NtgError, match="-4") as e:
        big.forms(dev(np.zeros((2, big.spec.nC))), [fm.square(0)], 1e-6)
    assert "LDS" in str(e.value)


# ---------------- 11. nothing existing moved ----------------
def test_the_neighbours_are_unchanged_by_a_forms_call():
    o4 = xo.inputs("O4")
    plan = api.Plan(o4.spec, 0)
    xd, lo, up = dev(o4.x[:5]), dev(o4.lower[:5]), dev(o4.upper[:5])
    s4 = po.inputs("S4")
    splan, sx, sp = api.Plan(s4.spec, 0), dev(s4.x), dev(s4.pairs[:9], torch.int32)

    def neighbours():
        return (cpu(plan.extrema(xd, o4.tol, lower=lo, upper=up)), cpu(plan.envelope_sos(xd, 1, lower=lo, upper=up)), cpu(splan.separation(sx, sp, s4.bodies, 0, tol=s4.tol)))

    before = neighbours()
    form = [fm.speed2(o4.spec, (0, 1)), fm.cross(o4.spec, (0, 1), (1, 1))]
    cpu(plan.forms(xd, form, 1e-6)); cpu(splan.forms(sx, form, 1e-6))
    after = neighbours()
    for a, b in zip(before, after):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
