"""-m gpu: ntg_batch_trig / Plan.trig -- certified extrema over the horizon of sums of sines and cosines of the flag declared at the call.

References: tests/trig_oracle.py (the definition in float64; that it encloses the sampled and polished extrema, and that the seeds leave its
decisions 16 slacks of room at 1e-6, is checked in tests/test_trig_oracle.py), the library's own ntg_batch_forms where a form is all LIN
(under ==), Plan.interp (the attained values) and Plan.check (the samples the certificate must dominate).  Slack: the header's rounding
statement, 2^-39 sum_t |w_t| (1 + A_t).  Shapes are small: 4 / 8 knot intervals (80 once, for the second pass over the intervals), 2 to 12
problems."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import trig_oracle as to
from cert_common import cpu
from gpu_common import dev
from ntg_amd import api, configs as cf, forms as fm, trig as tg

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
        self.c = c = to.inputs(name)
        self.name, self.nb, self.nform = name, c.x.shape[0], len(c.forms)
        self.spec = c.spec if family is None else dataclasses.replace(c.spec, family=family)
        self.plan = api.Plan(self.spec, 0)
        if c.knots is not None:
            self.plan.set_grids(dev(c.knots), dev(c.bps))
        self.xd, self.fd = dev(c.x), None if c.fprm is None else dev(c.fprm)
        self._runs = {}

    def bounds(self, tol):
        """bounds that cut through the forms' ranges: the medians over the batch of the attained minimum and maximum; the last form has none"""
        ext = np.array([[r["ext"] for r in row] for row in self.c.levels(tol)])
        lo, up = np.tile(np.nanmedian(ext[:, :, 1], axis=0), (self.nb, 1)), np.tile(np.nanmedian(ext[:, :, 2], axis=0), (self.nb, 1))
        lo[:, -1], up[:, -1] = -cf.INF_BOUND, cf.INF_BOUND
        return lo, up

    def run(self, tol, max_depth=30, bounds=False):
        key = (tol, max_depth, bounds)
        if key not in self._runs:
            kw = {}
            if bounds:
                lo, up = self.bounds(tol)
                kw = dict(lower=dev(lo), upper=dev(up))
            self._runs[key] = cpu(self.plan.trig(self.xd, self.c.forms, tol, max_depth, fprm=self.fd, **kw))
        return self._runs[key]


_cases = {}


def get_case(name, family=None):
    if name not in _cases:
        _cases[name] = Case(name, family)
    return _cases[name]


@pytest.fixture(scope="module", params=to.CASES)
def case(request):
    return get_case(request.param, request.getfixturevalue("module_family") if request.param == "TMOD" else None)


def same_as_oracle(got, ref, sl, label, knots=None):
    """status and npieces equal; ext and when within the slack.  knots: the case repeats one shape on every knot interval (L80), so its
    smallest and largest end values are ties between the knots, which rounding decides: the witness times are then only asked to be knots"""
    assert got["status"].tolist() == [[r["status"] for r in row] for row in ref], label
    assert got["npieces"].tolist() == [[r["npieces"] for r in row] for row in ref], label
    rext, rwhen = np.array([[r["ext"] for r in row] for row in ref]), np.array([[r["when"] for r in row] for row in ref])
    err = float((np.abs(got["ext"] - rext) / sl[:, :, None]).max())
    if knots is None:
        err = max(err, float((np.abs(got["when"] - rwhen) / sl[:, :, None]).max()))
    else:
        assert np.isin(got["when"], knots).all() and np.isin(rwhen, knots).all(), label
    print(f"{label}: ext and when differ from the oracle's by at most {err:.3g} slack; {got['npieces'].mean():.1f} pieces per form")
    assert err <= 1.0, label
    return rext


def oracle_violation(rext, lo, up):
    vw = [to.violation(rext[b], lo[b], up[b]) for b in range(len(rext))]
    return np.array([v for v, _ in vw]), np.array([w for _, w in vw])


# ---------------- 1. against the oracle at 1e-6: the decisions, the figures, the violation (6. TPP, TMOD, L80 are cases of it) ----------------
def test_against_the_oracle(case):
    c = case.c
    got = case.run(to.TOL, bounds=True)
    assert set(got) == set(KEYS + ("viol", "where"))
    rext = same_as_oracle(got, c.levels(to.TOL), c.sl, case.name, np.asarray(c.spec.knots[0]) if case.name == "L80" else None)
    assert (got["status"] == c.expect).all()
    if c.expect == to.OK:
        assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= to.TOL).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= to.TOL).all()
    lo, up = case.bounds(to.TOL)
    rv, rw = oracle_violation(rext, lo, up)
    err = float((np.abs(got["viol"] - rv) / c.sl.max(axis=1)[:, None]).max())
    print(f"{case.name}: viol differs from the oracle's by at most {err:.3g} slack; attained > 0 in {(got['viol'][:, 0] > 0).sum()} of {case.nb} problems")
    assert err <= 1.0 and np.array_equal(got["where"], rw)
    assert (got["viol"][:, 1] >= got["viol"][:, 0]).all() and (got["where"] != case.nform - 1).all()
    without = case.run(to.TOL)
    assert set(without) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(got[k], without[k]), k


# ---------------- 2. at 1e-9: the figures, and the attained values against Plan.interp ----------------
@pytest.mark.parametrize("name", ["TA4", "TE8", "TK8", "TD", "TPP"])
def test_at_1e_9(name):
    case = get_case(name)
    c, got = case.c, case.run(to.TOL9)
    ref = c.levels(to.TOL9)
    assert (got["status"] == to.OK).all()
    assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= to.TOL9).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= to.TOL9).all()
    rext = np.array([[r["ext"] for r in row] for row in ref])
    err = float((np.abs(got["ext"] - rext) / (to.TOL9 + c.sl[:, :, None])).max())
    print(f"{name}: ext differs from the oracle's by at most {err:.3g} (tol + slack); depth {max(r['depth'] for row in ref for r in row)}, "
          f"{got['npieces'].mean():.1f} pieces per form (oracle {np.mean([[r['npieces'] for r in row] for row in ref]):.1f})")
    assert err <= 1.0
    per = c.knots is not None
    t = got["when"].reshape(case.nb, -1)
    z = cpu({"z": case.plan.interp(case.xd, dev(t if per else t.reshape(-1)))})["z"]
    v = to.values(case.spec, z, c.forms, c.fprm)
    for b in range(case.nb):
        for f in range(case.nform):
            for s in range(2):
                at = 2 * f + s if per else (b * case.nform + f) * 2 + s
                assert abs(v[b, at, f] - got["ext"][b, f, 1 + s]) <= c.sl[b, f], (name, b, f, s)


# ---------------- 3. one call with every form equals the calls with one form each; 4. bit-identical ----------------
def test_forms_one_by_one_and_batch_independence():
    case = get_case("TA4")
    c, all12 = case.c, case.run(to.TOL)
    again = cpu(case.plan.trig(case.xd, c.forms, to.TOL, fprm=case.fd))
    one = cpu(case.plan.trig(dev(c.x[7:8]), c.forms, to.TOL, fprm=dev(c.fprm[7:8])))
    idx = [3, 7, 0, 11, 5]
    five = cpu(case.plan.trig(dev(c.x[idx]), c.forms, to.TOL, fprm=dev(c.fprm[idx])))
    big = cpu(case.plan.trig(dev(np.tile(c.x, (6, 1))), c.forms, to.TOL, fprm=dev(np.tile(c.fprm, (6, 1)))))   # 72 problems: several passes
    for k in KEYS:
        assert np.array_equal(all12[k], again[k]), k
        assert np.array_equal(one[k][0], all12[k][7]) and np.array_equal(five[k][1], all12[k][7]), k
        assert np.array_equal(big[k][60 + 7], all12[k][7]) and np.array_equal(big[k][:12], all12[k]), k
    for f in range(case.nform):
        single = cpu(case.plan.trig(case.xd, [c.forms[f]], to.TOL, fprm=case.fd))
        for k in KEYS:
            assert np.array_equal(single[k][:, 0], all12[k][:, f]), (k, f)


# ---------------- 5. the pin: all-LIN forms against Plan.forms, under == ----------------
@pytest.mark.parametrize("name", ["TD", "TK8", "TPP"])
def test_all_lin_forms_are_plan_forms(name):
    case = get_case(name)
    tforms, qforms = to.lin_pin_forms(case.spec)
    for tol in (to.TOL, to.TOL9):
        got, ref = cpu(case.plan.trig(case.xd, tforms, tol)), cpu(case.plan.forms(case.xd, qforms, tol))
        assert ref["npieces"].max() > case.spec.kninterv[0]
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), (k, tol, np.argwhere(got[k] != ref[k])[:6].tolist(), np.abs(got[k] - ref[k]).max())


# ---------------- 6. FULL, NAN, DEPTH ----------------
def test_full_nan_and_depth():
    full = get_case("TFULL")
    got, ref = full.run(to.TOL9), full.c.levels(to.TOL9)
    assert (got["status"] == to.FULL).all() and got["status"].tolist() == [[r["status"] for r in row] for row in ref]
    W = 1.0
    assert (got["ext"][:, :, 0] >= -W).all() and (got["ext"][:, :, 3] <= W).all()       # the clamp: a sine stays a sine
    rext = np.array([[r["ext"] for r in row] for row in ref])
    assert (got["ext"][:, :, 0] <= rext[:, :, 1] + full.c.sl).all() and (got["ext"][:, :, 3] >= rext[:, :, 2] - full.c.sl).all()
    nanc = get_case("TNAN")
    got, clean = nanc.run(to.TOL), cpu(nanc.plan.trig(dev(np.nan_to_num(nanc.c.x)), nanc.c.forms, to.TOL))
    assert (got["status"][1] == to.NAN).all() and np.isnan(got["ext"][1]).all() and np.isnan(got["when"][1]).all()
    for k in KEYS:
        assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]), k
    assert (got["status"][[0, 2]] == to.OK).all()
    td = get_case("TD")
    got, ref = td.run(to.TOL9, max_depth=3), td.c.levels(to.TOL9, 3)
    assert (got["status"] == to.DEPTH).any() and got["status"].tolist() == [[r["status"] for r in row] for row in ref]
    rext = np.array([[r["ext"] for r in row] for row in ref])
    assert (np.abs(got["ext"] - rext) <= to.TOL9 + td.c.sl[:, :, None]).all()


# ---------------- 7. the use: a solved manipulator, samples against the certificate ----------------
def test_certifying_a_solved_manipulator():
    spec = cf.config_E(ninterv=8, narms=2)
    nb, ceiling = 6, 2.5
    lo, up = cf.manipulator_bounds(nb, narms=2, ceiling=ceiling)
    plan = api.Plan(spec, 0)
    x = torch.ones((nb, spec.nC), dtype=torch.float64, device="cuda:0")
    out = plan.solve(dev(lo), dev(up), x, api.default_opts(hessian=3))
    torch.cuda.synchronize()
    assert (out["inform"].cpu().numpy() == 0).all()
    times = np.linspace(0.0, 5.0, 1001)
    chk = cpu(plan.check(x, dev(lo), dev(up), dev(times)))["viol"]
    forms = [tg.tip_height(spec, 0), tg.tip_height(spec, 1)]
    flo, fhi = np.full((nb, 2), -cf.INF_BOUND), np.full((nb, 2), ceiling)
    got = cpu(plan.trig(x, forms, to.TOL9, lower=dev(flo), upper=dev(fhi)))
    sl = to.slack(spec, x.cpu().numpy(), forms).max(axis=1)
    print("check at 1001 times:", chk, "\nattained:", got["viol"][:, 0], "\ncertified:", got["viol"][:, 1], "\npieces per form:", got["npieces"].mean())
    assert (got["status"] == to.OK).all()
    assert (got["viol"][:, 1] >= got["viol"][:, 0]).all() and (got["viol"][:, 0] >= chk - sl).all()
    assert (got["viol"][:, 1] - got["viol"][:, 0] <= to.TOL9).all()
    assert (chk > 0).any()       # the solver enforces the ceiling at the breakpoints only: between them the tips do pass it
    raised = cpu(plan.trig(x, forms, to.TOL9, lower=dev(flo), upper=dev(fhi + got["viol"][:, 1][:, None])))
    assert (raised["viol"][:, 1] == 0.0).all() and (raised["where"][:, 1] == -1).all()
    with pytest.raises(api.NtgError, match="-4"):      # ... and ntg_batch_extrema still refuses the plan
        plan.extrema(x, to.TOL9)


# ---------------- 8. refusals that need a plan ----------------
def test_refusals():
    case = get_case("TA4")
    c = case.c
    t0 = c.forms[0][0]
    x2, f2 = dev(c.x[:2]), dev(c.fprm[:2])
    lo = dev(np.zeros((2, 1)))
    assert set(cpu(case.plan.trig(x2, [c.forms[0]], to.TOL))) == set(KEYS)
    for forms, kw, rc, word in (([[t0._replace(kind=3)]], {}, "-2", "form 0, term 0: kind = 3"),
                                ([c.forms[0], [t0._replace(pp=1)]], dict(fprm=f2), "-2", "form 1, term 0: pp"),
                                ([[t0._replace(pp=0)]], {}, "-2", "form 0, term 0: pp"),
                                ([[t0._replace(ent=(9,))]], {}, "-2", "ent[0] = 9"),
                                ([[t0._replace(w=float("inf"))]], {}, "-2", "finite"),
                                ([[t0._replace(coef=(float("nan"),))]], {}, "-2", "finite"),
                                ([c.forms[0] * 2], {}, "-2", "form 0 has 6 terms"),
                                ([c.forms[0]] * 9, {}, "-2", "nform"),
                                ([c.forms[0]], dict(tol=-1.0), "-2", "tol"),
                                ([c.forms[0]], dict(max_depth=31), "-2", "max_depth"),
                                ([c.forms[0]], dict(sides=0), "-2", "sides")):
        kw = dict(dict(tol=to.TOL), **kw)
        with pytest.raises(api.NtgError, match=rc) as e:
            case.plan.trig(x2, forms, **kw)
        assert word in str(e.value), (word, str(e.value))
    L = api.lib()
    nt = (api.C.c_int * 1)(1)
    term = (api.TrigTerm * 1)(api.TrigTerm(0, 1, -1, 0, (api.C.c_int * 4)(0, 0, 0, 0), (api.C.c_double * 4)(1.0, 0, 0, 0), 0.0, 1.0))
    viol = torch.zeros((2, 2), dtype=torch.float64, device="cuda:0")
    raw = lambda lo_, up_, v: L.ntg_batch_trig(case.plan.h, 2, x2.data_ptr(), 1, nt, term, 0, None, 1e-6, 30, 3, lo_, up_, None, None, None, None, v, None, None)
    assert raw(None, None, viol.data_ptr()) == -2 and "bounds" in L.ntg_last_error().decode()     # violation outputs without bounds
    assert raw(lo.data_ptr(), None, viol.data_ptr()) == -2 and raw(lo.data_ptr(), lo.data_ptr(), viol.data_ptr()) == 0
    assert raw(None, None, None) == -2 and "no output" in L.ntg_last_error().decode()
    t3 = cf.config_T(nout=3, order=5, ninterv=4)   # outputs 0, 1 in one basis class, output 2 in another
    p3 = api.Plan(t3, 0)
    with pytest.raises(api.NtgError, match="-4") as e:
        p3.trig(dev(np.zeros((2, t3.nC))), [tg.heading(t3, 0, kind=tg.SIN), to.cross_class_form(t3)], to.TOL)
    assert "form 1 names outputs 0 and 2 of different basis classes" in str(e.value)
    pp = get_case("TPP")
    with pytest.raises(api.NtgError, match="-2") as e:      # a batch other than the grids'
        pp.plan.trig(dev(pp.c.x[:5]), pp.c.forms, to.TOL)
    assert "per-problem grids" in str(e.value)
    big = api.Plan(cf._kincar_spec(1, 6, 3, 340, 341, 5.0, "kincar-l340"), 0)   # 340 (36 + 2) + 1 doubles of tables and 2 (2046 + 64 * 27) of two waves: 160 KiB
    with pytest.raises(api.NtgError, match="-4") as e:
        big.trig(dev(np.zeros((2, big.spec.nC))), [tg.heading(big.spec, 0, kind=tg.SIN)], to.TOL)
    assert "LDS" in str(e.value)
