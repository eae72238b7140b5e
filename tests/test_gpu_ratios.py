"""-m gpu: ntg_batch_ratios / Plan.ratios -- certified extrema over the horizon of ratios of products of quadratic forms of the flag.

References: tests/ratios_oracle.py (the definition in float64; that it encloses the exact extrema, and the margins of its decisions to their
limits, are checked in tests/test_ratios_oracle.py), the library's own ntg_batch_forms where a ratio is one form (bit for bit), Plan.interp
(witness times and soundness) and ntg_batch_kincar_reverse (the steering angle).  Slack: the header's rounding statement.  Every ratio has its
own unit, so every ratio of a case has its own tolerances and is run in a call of its own, once at max(1e-9 of its largest quotient,
ratios_oracle.TOL_SLACKS slacks) and once at 1e-9 of its largest quotient, decision for decision against the oracle both times; one call with
all ratios is compared with those.  Shapes are small: 4 / 8 / 20 knot intervals, 6 to 24 problems."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import forms_oracle as fo
import ratios_oracle as ro
from cert_common import cpu, piece_times
from gpu_common import dev
from ntg_amd import api, configs as cf, forms as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ext", "when", "status", "npieces")
NONE = (-np.inf, np.inf, -np.inf, np.inf)


@pytest.fixture(scope="module")
def module_family():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))


class Case:
    def __init__(self, name, family=None):
        self.c = c = ro.inputs(name)
        self.name, self.nb, self.nratio = name, c.x.shape[0], len(c.ratios)
        self.spec = c.spec if family is None else dataclasses.replace(c.spec, family=family)
        self.plan = api.Plan(self.spec, 0)
        if c.knots is not None:
            self.plan.set_grids(dev(c.knots), dev(c.bps))
        self.xd = dev(c.x)
        # bounds that cut through the ratios' ranges: the medians over the batch of the attained minimum and maximum
        ext = np.array([[r["ext"] for r in row] for row in c.levels()])
        self.lo = np.tile(np.median(ext[:, :, 1], axis=0), (self.nb, 1)); self.up = np.tile(np.median(ext[:, :, 2], axis=0), (self.nb, 1))
        self._runs = {}

    def one(self, r, tol=None, max_depth=30, bounds=False, x=None):
        """ratio r in a call of its own, at its own tolerance"""
        key = (r, tol, max_depth, bounds)
        if x is not None or key not in self._runs:
            kw = dict(lower=dev(self.lo[:, r:r + 1]), upper=dev(self.up[:, r:r + 1])) if bounds else {}
            out = cpu(self.plan.ratios(self.xd if x is None else dev(x), self.c.forms, [self.c.ratios[r]], self.c.tol[r] if tol is None else tol, max_depth, **kw))
            if x is not None:
                return out
            self._runs[key] = out
        return self._runs[key]

    def each(self, fine=False, **kw):
        """every ratio in a call of its own, at its own tolerance (fine: 1e-9 of its largest quotient): the dict of one call with all of them"""
        outs = [self.one(r, **(dict(kw, tol=float(self.c.fine[r])) if fine else kw)) for r in range(self.nratio)]
        return {k: np.concatenate([o[k] for o in outs], axis=1) for k in KEYS}


_cases = {}


def get_case(name, family=None):
    if name not in _cases:
        _cases[name] = Case(name, family)
    return _cases[name]


@pytest.fixture(scope="module", params=ro.CASES)
def case(request):
    return get_case(request.param, request.getfixturevalue("module_family") if request.param == "RMOD" else None)


def same_as_oracle(got, ref, sl, label):
    """status and npieces equal; ext and when within the slack.  ref [nb][nratio] of level_oracle's dicts"""
    assert got["status"].tolist() == [[r["status"] for r in row] for row in ref], label
    assert got["npieces"].tolist() == [[r["npieces"] for r in row] for row in ref], label
    rext, rwhen = np.array([[r["ext"] for r in row] for row in ref]), np.array([[r["when"] for r in row] for row in ref])
    fin = np.isfinite(rext)
    assert np.array_equal(got["ext"][~fin], rext[~fin]), label
    err = float((np.abs(got["ext"] - rext) / sl[:, :, None])[fin].max())
    err = max(err, float((np.abs(got["when"] - rwhen) / sl[:, :, None]).max()))
    print(f"{label}: ext and when differ from the oracle's by at most {err:.3g} slack; {got['npieces'].mean():.1f} pairs per ratio")
    assert err <= 1.0, label
    return rext


# ---------------- 1. against the oracle, the violation figures, one call with every ratio ----------------
def test_against_the_oracle(case):
    c = case.c
    got = case.each()
    rext = same_as_oracle(got, c.levels(), c.sl, case.name)
    assert (got["status"] == ro.OK).all()
    assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= c.tol[None, :]).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= c.tol[None, :]).all()
    for r in range(case.nratio):
        with_b = case.one(r, bounds=True)
        assert set(with_b) == set(KEYS + ("viol", "where"))
        for k in KEYS:
            assert np.array_equal(with_b[k], case.one(r)[k]), k
        vw = [ro.violation(rext[b, r:r + 1], case.lo[b, r:r + 1], case.up[b, r:r + 1]) for b in range(case.nb)]
        rv, rw = np.array([v for v, _ in vw]), np.array([w for _, w in vw])
        err = float((np.abs(with_b["viol"] - rv) / c.sl[:, r:r + 1]).max())
        print(f"{case.name} ratio {r}: viol differs from the oracle's by at most {err:.3g} slack; attained > 0 in {(with_b['viol'][:, 0] > 0).sum()} of {case.nb} problems")
        assert err <= 1.0 and np.array_equal(with_b["where"], rw)
        assert (with_b["viol"][:, 1] >= with_b["viol"][:, 0]).all() and 0 < (with_b["viol"][:, 0] > 0).sum()
    # one call with every ratio at one tolerance: every ratio as in a call of its own at that tolerance, and the violation the largest of them
    tol = float(c.tol.max())
    both = cpu(case.plan.ratios(case.xd, c.forms, c.ratios, tol, lower=dev(case.lo), upper=dev(case.up)))
    alone = [cpu(case.plan.ratios(case.xd, c.forms, [c.ratios[r]], tol, lower=dev(case.lo[:, r:r + 1]), upper=dev(case.up[:, r:r + 1]))) for r in range(case.nratio)]
    for k in KEYS:
        assert np.array_equal(both[k], np.concatenate([a[k] for a in alone], axis=1)), k
    viols = np.stack([a["viol"] for a in alone], axis=2)   # [nb, 2, nratio]
    assert np.array_equal(both["viol"], viols.max(axis=2))
    assert np.array_equal(both["where"], np.where(viols.max(axis=2) > 0, viols.argmax(axis=2), -1))


# ---------------- 1b. decision for decision at 1e-9 of the largest quotient ----------------
def test_against_the_oracle_at_a_fine_tolerance(case):
    """Every case again at 1e-9 of every ratio's largest quotient: up to 26 levels deep, up to 47 pairs open at once (RK20), hundreds of pairs
    per ratio.  The margins of the oracle's decisions are far below the slack there, so equal status and npieces do not follow from the
    rounding statement: they are asserted because both sides run the definition's operations in IEEE double in the same order (they differ
    where the compiler contracts a multiply-add in the forms' builder), and a kernel that compacted the list or halved a pair wrongly would
    show here and nowhere else.  ext and when within one slack, as everywhere"""
    c = case.c
    ref = c.levels(c.fine)
    got = case.each(fine=True)
    same_as_oracle(got, ref, c.sl, case.name + " at 1e-9")
    assert (got["status"] == ro.OK).all()
    assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= c.fine[None, :]).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= c.fine[None, :]).all()
    most, deep = max(r["max_open"] for row in ref for r in row), max(r["depth"] for row in ref for r in row)
    print(f"{case.name} at 1e-9: most open {most}, depth {deep}, pairs per ratio up to {got['npieces'].max()}")
    assert deep >= 18 and got["npieces"].max() > 4 * c.spec.kninterv[0]
    if case.name == "RK20":
        assert 40 <= most <= ro.xo.CAP


# ---------------- 2. bit for bit against code that exists today ----------------
@pytest.mark.parametrize("name", ["K4", "PP"])
def test_bit_for_bit_a_single_form_over_one(name):
    f = fo.inputs(name)
    plan = api.Plan(f.spec, 0)
    if f.knots is not None:
        plan.set_grids(dev(f.knots), dev(f.bps))
    xd, fd = dev(f.x), None if f.fprm is None else dev(f.fprm)
    ref = cpu(plan.forms(xd, f.forms, f.tol, fprm=fd))
    assert (ref["npieces"] > f.spec.kninterv[0]).any()
    for f0 in range(0, len(f.forms), api.RATIO_MAXRATIOS):
        idx = list(range(f0, min(f0 + api.RATIO_MAXRATIOS, len(f.forms))))
        got = cpu(plan.ratios(xd, f.forms, [fm.ratio([i]) for i in idx], f.tol, fprm=fd))
        for k in KEYS:
            assert np.array_equal(got[k], ref[k][:, idx], equal_nan=True), (k, idx)
    one = cpu(plan.ratios(xd, f.forms, [fm.ratio([0], [0])], f.tol, fprm=fd))   # S / S
    assert (one["ext"] == 1.0).all() and (one["status"] == ro.OK).all()
    # no pair opens where the polygons of S are positive: npieces == l.  (Where y' changes sign the product polygon of y'^2 dips below zero, S's
    # with it on some of these cars, and rule 2 opens such a pair until its halves are positive.)
    positive = f.polys[0].reshape(f.x.shape[0], -1).min(axis=1) > 0.0
    assert positive.sum() >= 4 and (one["npieces"][positive, 0] == f.spec.kninterv[0]).all() and (one["npieces"][~positive, 0] > f.spec.kninterv[0]).all()


# ---------------- 3. soundness against samples, and the witness times ----------------
@pytest.mark.parametrize("name", ["RK4", "RPP", "R8"])
def test_samples_lie_inside_and_the_witness_times_attain(name):
    case = get_case(name)
    c, got = case.c, case.each()
    per = c.knots is not None
    for r in range(case.nratio):
        ends = np.stack([np.asarray(c.kn(b, r), dtype=np.float64) for b in range(case.nb if per else 1)])
        t = np.stack([piece_times(e).reshape(-1) for e in ends])
        t = np.concatenate([t, got["when"][:, r, :] if per else got["when"][:, r, :].reshape(1, -1)], axis=1)
        z = cpu({"z": case.plan.interp(case.xd, dev(t if per else t[0]))})["z"]
        v = ro.values(case.spec, z, c.forms, c.ratios, c.fprm)[:, :, r]
        sl = c.sl[:, r][:, None]
        ns = t.shape[1] - (2 if per else 2 * case.nb)
        assert (v[:, :ns] >= got["ext"][:, r, 0][:, None] - sl).all() and (v[:, :ns] <= got["ext"][:, r, 3][:, None] + sl).all(), (name, r)
        w = v[:, ns:] if per else np.stack([v[b, ns + 2 * b:ns + 2 * b + 2] for b in range(case.nb)])
        err = float((np.abs(w - got["ext"][:, r, 1:3]) / sl).max())
        print(f"{name} ratio {r}: the values at the witness times differ from min_hi / max_lo by at most {err:.3g} slack")
        assert err <= 1.0, (name, r)


# ---------------- 4. the steering certificate, end to end; the work list near its cap ----------------
def test_tight_steering_certificate_of_the_kinematic_car():
    case = get_case("RK20")
    c = case.c
    L = 3.0
    forms, kappa2 = fm.curvature2(c.spec, (0, 1))
    assert forms == c.forms[:2] and kappa2 == c.ratios[0]
    tol = float(c.fine[0])   # 1e-9 of the largest kappa^2: test_against_the_oracle_at_a_fine_tolerance compares this run with the oracle
    got = case.one(0, tol=tol)
    tan_max = fm.steering_tan_max(got, L)
    fext = cpu(case.plan.forms(case.xd, forms, 1e-6))["ext"]
    loose = fm.steering_bound(fext, L)
    print("RK20: loose / tight certified |tan delta|", np.round(loose / tan_max, 2))
    assert np.isfinite(tan_max).all() and (tan_max <= loose * (1.0 + 1e-9)).all()
    kn = np.asarray(c.spec.knots[0])
    t = np.unique(np.clip((kn[:-1, None] + np.diff(kn)[:, None] * np.linspace(0.0, 1.0, 33)[None, :]).reshape(-1), kn[0], kn[-1]))
    z = case.plan.interp(case.xd, dev(np.concatenate([t, got["when"][:, 0, 1]])))
    state = cpu({"s": case.plan.kincar_reverse(z, wheelbase=L)})["s"]     # [nb, nt, 1, 5] = x, y, theta, v, delta
    tan = np.tan(state[:, :, 0, 4])
    sl_tan = L * np.sqrt(c.sl[:, 0])   # |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)
    assert (np.abs(tan[:, :t.size]).max(axis=1) <= tan_max + sl_tan).all()
    at = np.array([tan[b, t.size + b] for b in range(case.nb)])
    err = float((np.abs(at * at - L * L * got["ext"][:, 0, 2]) / (L * L * c.sl[:, 0])).max())
    print(f"RK20: tan^2 delta of kincar_reverse at t_max differs from L^2 max_lo by at most {err:.3g} slack")
    assert err <= 1.0
    assert fm.steering_tan_max({"ext": got["ext"], "status": np.full_like(got["status"], ro.POLE)}, L).tolist() == [np.inf] * case.nb


# ---------------- 5. POLE ----------------
def test_a_parked_car_is_a_pole_and_nobody_else_notices():
    case = get_case("RK4")
    c = case.c
    x = c.x.copy()
    n = c.spec.ncoef[0]
    x[7, 3:9] = x[7, 3]; x[7, n + 3:n + 9] = x[7, n + 3]   # the six coefficients of knot interval 1, of x and of y: the car stands still on it
    for r in range(case.nratio):
        clean = case.one(r, bounds=True)
        kw = dict(lower=dev(case.lo[:, r:r + 1]), upper=dev(case.up[:, r:r + 1]))
        got = cpu(case.plan.ratios(dev(x), c.forms, [c.ratios[r]], c.tol[r], **kw))
        for k in KEYS + ("viol", "where"):
            assert np.array_equal(np.delete(got[k], 7, axis=0), np.delete(clean[k], 7, axis=0)), (r, k)
        if c.ratios[r][1]:
            assert got["status"][7, 0] == api.RATIO_POLE and tuple(got["ext"][7, 0]) == NONE and np.isnan(got["when"][7, 0]).all()
            assert got["npieces"][7, 0] == c.spec.kninterv[0]
            assert got["viol"][7].tolist() == [0.0, np.inf] and got["where"][7].tolist() == [-1, 0]
        else:
            assert got["status"][7, 0] != api.RATIO_POLE and got["ext"][7, 0, 1] == 0.0   # S S has no denominator: its minimum 0 is attained


# ---------------- 6. DEPTH ----------------
def test_depth():
    case = get_case("RK4")
    c = case.c
    kn = np.asarray(c.spec.knots[0])
    xp = fm.entry(c.spec, 0, 1)
    tq = kn[1] + (kn[2] - kn[1]) / 3.0
    cval = cpu({"z": case.plan.interp(case.xd, dev(np.array([tq])))})["z"][:, 0, xp]   # x' at local parameter 1/3 of knot interval 1
    forms, ratio = [fm.square(xp, param=0)], ([], [0])   # 1 / (x' - c)^2: the denominator touches zero between the ends the bisection visits
    fprm = cval[:, None].copy()
    # (16 levels: the nearest end visited is then 1e-5 of the interval from the root, the denominator there 1e-11, far above the 1e-16 its
    # points carry from the halvings; at 30 levels the sign of an end next to the root would be noise, POLE here and DEPTH there)
    got = cpu(case.plan.ratios(case.xd, forms, [ratio], 1e-6, 16, fprm=dev(fprm)))
    d = ro.Inputs("touch", c.spec, c.x, forms, [ratio], fprm=fprm)
    d.pairs = ro.pair_polygons(c.spec, c.x, forms, [ratio], fprm)
    ref = [[ro.level_oracle(d.pairs[0][0][b], d.pairs[0][1][b], kn, 1e-6, 16)] for b in range(case.nb)]
    assert got["status"].tolist() == [[r[0]["status"]] for r in ref]
    assert (got["status"] == ro.DEPTH).all() and np.isposinf(got["ext"][:, 0, 3]).all() and np.isfinite(got["ext"][:, 0, 1:3]).all()
    assert got["npieces"].tolist() == [[r[0]["npieces"]] for r in ref]
    # the attained figures and their times against the oracle's: the smallest quotient 1 / d_max and the largest one, 1 / d at the visited end
    # next to the root, each within the statement's slack at its own denominator where it is finite
    d.fsl, d.fpolys = fo.slack(c.spec, c.x, forms, fprm), fo.form_polygons(c.spec, c.x, forms, fprm)
    for b in range(case.nb):
        for i in (1, 2):
            q = ref[b][0]["ext"][i]
            sl = ro.slack_of(d, b, 0, q, 1.0 / q)
            if np.isfinite(sl):
                assert abs(got["ext"][b, 0, i] - q) <= sl and abs(got["when"][b, 0, i - 1] - ref[b][0]["when"][i - 1]) <= sl, (b, i)
            else:   # next to the root the denominator is below its eps: the statement claims no figure there, but the visited end is the same one
                assert i == 2 and got["when"][b, 0, 1] == ref[b][0]["when"][1] and got["ext"][b, 0, 2] > 0.0, (b, i)
    # max_depth = 3: a finite enclosure that contains the one of depth 30
    deep, flat = case.each(), case.each(max_depth=3)
    same_as_oracle(flat, c.levels(max_depth=3), c.sl, "RK4, max_depth 3")
    assert (flat["status"] == ro.DEPTH).sum() >= case.nb and set(np.unique(flat["status"])) <= {ro.OK, ro.DEPTH} and np.isfinite(flat["ext"]).all()
    assert (flat["ext"][:, :, 0] <= deep["ext"][:, :, 0] + c.sl).all() and (flat["ext"][:, :, 3] >= deep["ext"][:, :, 3] - c.sl).all()


# ---------------- 7. NaN ----------------
def test_nan_marks_the_ratios_that_name_it():
    case = get_case("RK4")
    c = case.c
    ratios = [ro.KAPPA2, ro.SLOPE, fm.ratio([2]), fm.ratio([2, 2], [2])]   # the last two name x' alone
    named = np.array([True, True, False, False])
    x = c.x.copy()
    x[5, c.spec.ncoef[0] + 1] = np.nan   # a coefficient of y on the first knot interval of problem 5
    tol = float(c.tol[0])
    got, ref = cpu(case.plan.ratios(dev(x), c.forms, ratios, tol)), cpu(case.plan.ratios(case.xd, c.forms, ratios, tol))
    for k in KEYS:
        assert np.array_equal(np.delete(got[k], 5, axis=0), np.delete(ref[k], 5, axis=0)), k
        assert np.array_equal(got[k][5, ~named], ref[k][5, ~named]), k
    assert (got["status"][5, named] == ro.NAN).all() and np.isnan(got["ext"][5, named]).all() and np.isnan(got["when"][5, named]).all()
    assert (ref["status"] == ro.OK).all()


# ---------------- 8. batch independence and repeatability ----------------
def test_batch_independence_and_repeatability():
    case = get_case("RK4")
    c = case.c
    all24 = case.one(0)
    again = case.one(0, x=c.x)
    one = case.one(0, x=c.x[19:20])
    five = case.one(0, x=c.x[[3, 19, 7, 0, 11]])
    for k in KEYS:
        assert np.array_equal(all24[k], again[k]), k
        assert np.array_equal(one[k][0], all24[k][19]) and np.array_equal(five[k][1], all24[k][19]), k


# ---------------- 9. refusals that need a plan ----------------
def test_refusals():
    case = get_case("RK4")
    c = case.c
    x2 = dev(c.x[:2])
    for ratios, code, words in (([([1, 1, 1, 1], [])], "-4", "ratio 0: its numerator has degree 28, above 24"),
                                ([ro.KAPPA2, ([0], [1, 1, 1, 1])], "-4", "ratio 1: its denominator has degree 28"),
                                ([([4], [])], "-2", "ratio 0 names form 4: the call declares forms 0 .. 3"),
                                ([ro.KAPPA2, ([0], [-1])], "-2", "ratio 1 names form -1"),
                                ([([], [])], "-2", "ratio 0 has both sides empty"),
                                ([ro.KAPPA2] * 5, "-2", "nratio must lie in 0 .. 4")):
        with pytest.raises(api.NtgError, match=code) as e:
            case.plan.ratios(x2, c.forms, ratios, 1e-6)
        assert words in str(e.value), (ratios, str(e.value))
    with pytest.raises(api.NtgError, match="-2") as e:   # the forms' own refusals come first, with their messages
        case.plan.ratios(x2, [c.forms[0], []], [ro.KAPPA2], 1e-6)
    assert "form 1 has 0 terms" in str(e.value)
    with pytest.raises(api.NtgError, match="-2") as e:
        case.plan.ratios(x2, c.forms, [ro.KAPPA2], -1.0)
    assert "tol" in str(e.value)
    empty = case.plan.ratios(x2, c.forms, [], 1e-6)   # nratio == 0: 0 after the checks
    assert set(empty) == set(KEYS)
    t4 = fo.inputs("T4")   # outputs 0, 1 in one basis class, output 2 in another
    tplan = api.Plan(t4.spec, 0)
    e0, e2 = fm.linear(fm.entry(t4.spec, 0, 0), 1.0), fm.square(fm.entry(t4.spec, 2, 0), shift=3.0)
    with pytest.raises(api.NtgError, match="-4") as e:
        tplan.ratios(dev(t4.x), [e0, e2], [fm.ratio([0], [1])], 1e-6)
    assert "ratio 0 names forms 0 and 1 of different basis classes" in str(e.value)
    ok = cpu(tplan.ratios(dev(t4.x), [e0, e2], [fm.ratio([0]), fm.ratio([], [1])], 1e-6))   # different ratios may use different classes
    assert (ok["status"][:, 0] == ro.OK).all()
    with pytest.raises(api.NtgError, match="-4") as e:      # a form across the classes is refused as ntg_batch_forms refuses it
        tplan.ratios(dev(t4.x), [e0, fo.cross_class_form(t4.spec)], [fm.ratio([0])], 1e-6)
    assert "form 1 names outputs 0 and 2 of different basis classes" in str(e.value)
    big = api.Plan(cf._kincar_spec(1, 6, 3, 300, 301, 5.0, "kincar-l300"), 0)
    with pytest.raises(api.NtgError, match="-4") as e:
        big.ratios(dev(np.zeros((2, big.spec.nC))), [fm.square(0)], [fm.ratio([0])], 1e-6)
    assert "LDS" in str(e.value)


# ---------------- 10. workgroups of two waves ----------------
def test_two_waves_where_four_work_lists_do_not_fit():
    """100 knot intervals: the class tables (3801 doubles) and four waves' rows and work lists (4 x 3870) pass 158 KiB, two waves' do not.
    Five problems: three passes of a workgroup, the last one partial; more than 64 intervals: level 0 takes two rounds over them and forms every
    pair twice.  Decision for decision against the oracle at the case's tolerance (the seed keeps 16 slacks of margin), and at 1e-9, where the
    work list overflows; every problem also alone, bit for bit"""
    spec = cf._kincar_spec(1, 6, 3, 100, 501, 5.0, "kincar-2out-k6-l100")
    forms, kappa2 = fm.curvature2(spec, (0, 1))
    c = ro.Inputs("RK100", spec, fo.kincar_x(spec, 5, 13, 0.002, 0.006), forms, [kappa2]).finish()   # (perturbations that leave x' = 8 +- 0.2 on intervals of 0.05 s)
    plan = api.Plan(spec, 0)
    lv = c.levels()
    assert all(r[0]["margin"] >= 16.0 * c.sl[b, 0] and r[0]["status"] == ro.OK and r[0]["npieces"] > 100 for b, r in enumerate(lv))   # (the seed's doing)
    tol = float(c.tol[0])
    got = cpu(plan.ratios(dev(c.x), forms, [kappa2], tol))
    same_as_oracle(got, lv, c.sl, "RK100")
    # at 1e-9 of the largest quotient 99 of the 100 intervals are open at level 0 (every interval of these weaving cars has a peak like the
    # others): the list overflows, status FULL with the hull of the level-0 pairs, as the oracle has it
    full = cpu(plan.ratios(dev(c.x), forms, [kappa2], float(c.fine[0])))
    same_as_oracle(full, c.levels(c.fine), c.sl, "RK100 at 1e-9")
    assert (full["status"] == ro.FULL).all() and (full["npieces"] == 100).all()
    for b in (0, 4):
        one = cpu(plan.ratios(dev(c.x[b:b + 1]), forms, [kappa2], tol))
        for k in KEYS:
            assert np.array_equal(one[k][0], got[k][b], equal_nan=True), (b, k)
