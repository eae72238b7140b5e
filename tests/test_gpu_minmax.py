"""-m gpu: ntg_batch_minmax / Plan.minmax -- certified extrema over the horizon of min / max expressions over forms declared at the call.

References: tests/minmax_oracle.py (the definition in float64; that it encloses the sampled and polished extrema, and that the seeds leave its
decisions and its `which` ties 16 slacks of room at 1e-6, is checked in tests/test_minmax_oracle.py), the library's own ntg_batch_forms on the
members (under == for a single member, within tol + slack for the lattice), Plan.interp (the attained values and the samples the certificate
must dominate).  Slack: the header's rounding statement, max over the members of 2^-39 (M_f + |d|).  Shapes are small: 4 / 8 / 20 knot
intervals (80 once, for the second pass over the intervals), 2 to 12 problems."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import forms_oracle as fo
import minmax_oracle as mo
from cert_common import cpu
from gpu_common import dev
from ntg_amd import api, configs as cf, forms as fm, minmax as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ext", "when", "status", "npieces")
KEYSW = KEYS + ("which",)


@pytest.fixture(scope="module")
def module_family():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))


class Case:
    def __init__(self, name, family=None):
        self.c = c = mo.inputs(name)
        self.name, self.nb, self.ngroup = name, c.x.shape[0], len(c.groups)
        self.spec = c.spec if family is None else dataclasses.replace(c.spec, family=family)
        self.plan = api.Plan(self.spec, 0)
        if c.knots is not None:
            self.plan.set_grids(dev(c.knots), dev(c.bps))
        self.xd, self.fd = dev(c.x), None if c.fprm is None else dev(c.fprm)
        self._runs = {}

    def bounds(self, tol):
        """bounds that cut through the groups' ranges: the medians over the batch of the attained minimum and maximum; the last group of
        several has none"""
        ext = np.array([[r["ext"] for r in row] for row in self.c.levels(tol)])
        lo, up = np.tile(np.nanmedian(ext[:, :, 1], axis=0), (self.nb, 1)), np.tile(np.nanmedian(ext[:, :, 2], axis=0), (self.nb, 1))
        if self.ngroup > 1:
            lo[:, -1], up[:, -1] = -cf.INF_BOUND, cf.INF_BOUND
        return lo, up

    def run(self, tol, max_depth=30, bounds=False):
        key = (tol, max_depth, bounds)
        if key not in self._runs:
            kw = {}
            if bounds:
                lo, up = self.bounds(tol)
                kw = dict(lower=dev(lo), upper=dev(up))
            self._runs[key] = cpu(self.plan.minmax(self.xd, self.c.forms, self.c.groups, tol, max_depth, fprm=self.fd, **kw))
        return self._runs[key]


_cases = {}


def get_case(name, family=None):
    if name not in _cases:
        _cases[name] = Case(name, family)
    return _cases[name]


@pytest.fixture(scope="module", params=mo.CASES)
def case(request):
    return get_case(request.param, request.getfixturevalue("module_family") if request.param == "MMOD" else None)


def same_as_oracle(got, ref, sl, label):
    """status, npieces and which equal; ext and when within the slack"""
    for k in ("status", "npieces"):
        assert got[k].tolist() == [[r[k] for r in row] for row in ref], (label, k)
    assert got["which"].tolist() == [[list(r["which"]) for r in row] for row in ref], label
    rext, rwhen = np.array([[r["ext"] for r in row] for row in ref]), np.array([[r["when"] for r in row] for row in ref])
    err = max(float((np.abs(got["ext"] - rext) / sl[:, :, None]).max()), float((np.abs(got["when"] - rwhen) / sl[:, :, None]).max()))
    print(f"{label}: ext and when differ from the oracle's by at most {err:.3g} slack; {got['npieces'].mean():.1f} pieces per group")
    assert err <= 1.0, label
    return rext


def oracle_violation(rext, lo, up):
    vw = [mo.violation(rext[b], lo[b], up[b]) for b in range(len(rext))]
    return np.array([v for v, _ in vw]), np.array([w for _, w in vw])


# ---------------- 1. against the oracle at 1e-6: the decisions, the figures, which, the violation ----------------
def test_against_the_oracle(case):
    c = case.c
    got = case.run(mo.TOL, bounds=True)
    assert set(got) == set(KEYSW + ("viol", "where"))
    rext = same_as_oracle(got, c.levels(mo.TOL), c.sl, case.name)
    assert (got["status"] == c.expect).all()
    assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= mo.TOL).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= mo.TOL).all()
    lo, up = case.bounds(mo.TOL)
    rv, rw = oracle_violation(rext, lo, up)
    err = float((np.abs(got["viol"] - rv) / c.sl.max(axis=1)[:, None]).max())
    print(f"{case.name}: viol differs from the oracle's by at most {err:.3g} slack; attained > 0 in {(got['viol'][:, 0] > 0).sum()} of {case.nb} problems")
    assert err <= 1.0 and np.array_equal(got["where"], rw)
    assert (got["viol"][:, 1] >= got["viol"][:, 0]).all() and (got["viol"][:, 0] > 0).any()
    if case.ngroup > 1:
        assert (got["where"] != case.ngroup - 1).all()
    without = case.run(mo.TOL)
    assert set(without) == set(KEYSW)
    for k in KEYSW:
        assert np.array_equal(got[k], without[k]), k


# ---------------- 2. at 1e-9: the figures, and the attained values against Plan.interp through the members' values ----------------
@pytest.mark.parametrize("name", mo.CASES9)
def test_at_1e_9(name):
    case = get_case(name)
    c, got = case.c, case.run(mo.TOL9)
    ref = c.levels(mo.TOL9)
    assert (got["status"] == mo.OK).all()
    assert (got["ext"][:, :, 1] - got["ext"][:, :, 0] <= mo.TOL9).all() and (got["ext"][:, :, 3] - got["ext"][:, :, 2] <= mo.TOL9).all()
    rext = np.array([[r["ext"] for r in row] for row in ref])
    err = float((np.abs(got["ext"] - rext) / (mo.TOL9 + c.sl[:, :, None])).max())
    print(f"{name}: ext differs from the oracle's by at most {err:.3g} (tol + slack); depth {max(r['depth'] for row in ref for r in row)}, "
          f"{got['npieces'].mean():.1f} pieces per group (oracle {np.mean([[r['npieces'] for r in row] for row in ref]):.1f})")
    assert err <= 1.0
    t = got["when"].reshape(-1)
    z = cpu({"z": case.plan.interp(case.xd, dev(t))})["z"]
    for g in range(case.ngroup):
        mv = mo.member_values(case.spec, z, c.forms, c.groups[g], c.fprm)
        for b in range(case.nb):
            for s in range(2):
                at = (b * case.ngroup + g) * 2 + s
                assert abs(mo.fold(c.groups[g], mv[b, at]) - got["ext"][b, g, 1 + s]) <= c.sl[b, g], (name, b, g, s)
                assert abs(mv[b, at, got["which"][b, g, s]] - got["ext"][b, g, 1 + s]) <= c.sl[b, g], (name, b, g, s)


# ---------------- 3. one call with every group equals the calls with one group each; bit-identical whatever the batch ----------------
def test_groups_one_by_one_and_batch_independence():
    case = get_case("MP4")
    c, all12 = case.c, case.run(mo.TOL)
    call = lambda x, f, groups=c.groups: cpu(case.plan.minmax(dev(x), c.forms, groups, mo.TOL, fprm=dev(f)))
    again, one = call(c.x, c.fprm), call(c.x[7:8], c.fprm[7:8])
    idx = [3, 7, 0, 11, 5]
    five = call(c.x[idx], c.fprm[idx])
    big = call(np.tile(c.x, (6, 1)), np.tile(c.fprm, (6, 1)))   # 72 problems: several passes
    for k in KEYSW:
        assert np.array_equal(all12[k], again[k]), k
        assert np.array_equal(one[k][0], all12[k][7]) and np.array_equal(five[k][1], all12[k][7]), k
        assert np.array_equal(big[k][60 + 7], all12[k][7]) and np.array_equal(big[k][:12], all12[k]), k
    for g in range(case.ngroup):
        single = call(c.x, c.fprm, [c.groups[g]])
        for k in KEYSW:
            assert np.array_equal(single[k][:, 0], all12[k][:, g]), (k, g)


# ---------------- 4. the three pins, under ==, at both tolerances ----------------
@pytest.mark.parametrize("name", ["MP4", "MK8", "MPP"])
def test_single_and_repeated_members_are_plan_forms(name):
    case = get_case(name)
    c = case.c
    nf = min(len(c.forms), 8)   # (Plan.forms takes 8 forms)
    for tol in (mo.TOL, mo.TOL9):
        ref = cpu(case.plan.forms(case.xd, c.forms[:nf], tol, fprm=case.fd))
        assert ref["npieces"].max() > case.spec.kninterv[0]
        for f0 in range(0, nf, 4):
            fs = list(range(f0, min(f0 + 4, nf)))
            for make in (mo.single_member, lambda f: (mo.MIN, mo.MAX, [[(f, 0.0, -1)], [(f, 0.0, -1)]]), lambda f: (mo.MAX, mo.MIN, [[(f, 0.0, -1), (f, 0.0, -1)]])):
                got = cpu(case.plan.minmax(case.xd, c.forms, [make(f) for f in fs], tol, fprm=case.fd))
                for k in KEYS:
                    assert np.array_equal(got[k], ref[k][:, fs]), (k, tol, fs, np.argwhere(got[k] != ref[k][:, fs])[:6].tolist())
                assert (got["which"] == 0).all()


@pytest.mark.parametrize("name", ["MP4", "MQ8", "MK8"])
def test_negation_swaps_min_and_max(name):
    case = get_case(name)
    c = case.c
    nf, ng, nfp = mo.negated(c.forms, c.groups, c.fprm)
    for tol in (mo.TOL, mo.TOL9):
        got, neg = case.run(tol), cpu(case.plan.minmax(case.xd, nf, ng, tol, fprm=None if nfp is None else dev(nfp)))
        assert np.array_equal(neg["ext"], -got["ext"][:, :, ::-1]) and np.array_equal(neg["when"], got["when"][:, :, ::-1]), tol
        assert np.array_equal(neg["which"], got["which"][:, :, ::-1]) and np.array_equal(neg["status"], got["status"]) and np.array_equal(neg["npieces"], got["npieces"]), tol


# ---------------- 5. lattice sanity against Plan.forms on the members ----------------
@pytest.mark.parametrize("name", ["MP4", "MQ8", "MK8", "MPP"])
def test_lattice_against_the_members(name):
    """pure MIN and pure MAX groups against their members' own certificates, within tol + slack: min_hi of MIN is the smallest member
    min_hi, max_lo of MAX the largest member max_lo, and min_lo of MAX is below no member's min_lo"""
    case = get_case(name)
    c, tol = case.c, mo.TOL
    got = case.run(tol)
    seen = 0
    for g, (outer, inner, clauses) in enumerate(c.groups):
        mem = mo.members(c.groups[g])[0]
        if not (outer == inner or len(clauses) == 1) or len(mem) > 8:
            continue
        kind = inner if len(clauses) == 1 else outer
        forms = [c.forms[f] for f, _, _ in mem]
        d = mo.offsets(c.groups[g], c.fprm, case.nb)
        ref = cpu(case.plan.forms(case.xd, forms, tol, fprm=case.fd))["ext"] + d[:, :, None]
        sl = (tol + c.sl[:, g])
        if kind == mo.MIN:
            assert (np.abs(got["ext"][:, g, 1] - ref[:, :, 1].min(axis=1)) <= sl).all(), (name, g)
        else:
            assert (np.abs(got["ext"][:, g, 2] - ref[:, :, 2].max(axis=1)) <= sl).all(), (name, g)
            assert (got["ext"][:, g, 0][:, None] >= ref[:, :, 0] - sl[:, None]).all(), (name, g)
        seen += 1
    assert seen > 0


# ---------------- 6. FULL, NAN, DEPTH ----------------
def test_full_nan_and_depth():
    full = get_case("MFULL")
    got, ref = full.run(mo.TOL9), full.c.levels(mo.TOL9)
    assert (got["status"] == mo.FULL).all() and got["status"].tolist() == [[r["status"] for r in row] for row in ref]
    rext = np.array([[r["ext"] for r in row] for row in ref])
    assert (np.abs(got["ext"] - rext) <= full.c.sl[:, :, None]).all() and got["npieces"].tolist() == [[r["npieces"] for r in row] for row in ref]
    nanc = get_case("MNAN")
    got, clean = nanc.run(mo.TOL), cpu(nanc.plan.minmax(dev(np.nan_to_num(nanc.c.x)), nanc.c.forms, nanc.c.groups, mo.TOL, fprm=nanc.fd))
    assert (got["status"][1] == mo.NAN).all() and np.isnan(got["ext"][1]).all() and np.isnan(got["when"][1]).all() and (got["which"][1] == -1).all()
    for k in KEYSW:
        assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]), k
    assert (got["status"][[0, 2]] == mo.OK).all()
    mq = get_case("MQ8")   # a kink at max_depth = 3
    got, ref = mq.run(mo.TOL9, max_depth=3), mq.c.levels(mo.TOL9, 3)
    assert (got["status"] == mo.DEPTH).any() and got["status"].tolist() == [[r["status"] for r in row] for row in ref]
    rext = np.array([[r["ext"] for r in row] for row in ref])
    assert (np.abs(got["ext"] - rext) <= mo.TOL9 + mq.c.sl[:, :, None]).all()
    assert (got["ext"][:, :, 0] <= got["ext"][:, :, 1]).all() and (got["ext"][:, :, 1] - got["ext"][:, :, 0] > mo.TOL9).any()   # valid, and honestly wide


# ---------------- 7. the use: a solved obstacle batch, samples against the certificate ----------------
def test_certifying_a_square_inside_the_obstacle_disc():
    spec = cf.config_O(ninterv=8)
    nb, tol = 6, mo.TOL
    lo, up = cf.obstacle_bounds(nb)
    plan = api.Plan(spec, 0)
    x = torch.ones((nb, spec.nC), dtype=torch.float64, device="cuda:0")
    plan.solve(dev(lo), dev(up), x, api.default_opts())
    torch.cuda.synchronize()
    forms, group = mm.polygon(spec, 0, 1, [(23.0, 0.5), (20.0, 3.5), (17.0, 0.5), (20.0, -2.5)])   # inscribed in the disc: centre (20, 0.5), half-diagonal 3
    glo, ghi = np.zeros((nb, 1)), np.full((nb, 1), cf.INF_BOUND)                                    # outside: min over t of max over faces >= 0
    got = cpu(plan.minmax(x, forms, [group], tol, lower=dev(glo), upper=dev(ghi)))
    xs = x.cpu().numpy()
    sl = mo.slack(spec, xs, forms, [group])[:, 0]
    times = np.linspace(0.0, 5.0, 1001)
    z = cpu({"z": plan.interp(x, dev(times))})["z"]
    pen = np.maximum(-mo.values(spec, z, forms, [group])[:, :, 0], 0.0).max(axis=1)
    print("penetration at 1001 times:", pen, "\nattained:", got["viol"][:, 0], "\ncertified:", got["viol"][:, 1], "\nstatus:", got["status"][:, 0], "pieces:", got["npieces"][:, 0])
    assert (got["status"] == mo.OK).all()
    assert (pen <= got["viol"][:, 0] + sl).all()
    assert (got["viol"][:, 1] >= got["viol"][:, 0]).all() and (got["viol"][:, 1] - got["viol"][:, 0] <= tol).all()
    pushed = cpu(plan.minmax(x, forms, [group], tol, lower=dev(glo - got["viol"][:, 1][:, None]), upper=dev(ghi)))
    assert (pushed["viol"][:, 1] == 0.0).all() and (pushed["where"][:, 1] == -1).all()


# ---------------- 8. refusals that need a plan ----------------
def test_refusals():
    case = get_case("MP4")
    c = case.c
    x2, f2 = dev(c.x[:2]), dev(c.fprm[:2])
    g0 = c.groups[1]   # the box: forms 3 .. 6, no parameter
    m0 = g0[2][0][0]
    assert set(cpu(case.plan.minmax(x2, c.forms, [g0], mo.TOL, fprm=f2))) == set(KEYSW)
    t0 = c.forms[3][0]
    many = [fm.linear(0, 1.0)] * 17
    for forms, groups, kw, rc, word in ((c.forms, [(2, 1, g0[2])], {}, "-2", "group 0: outer and inner"),
                                        (c.forms, [(0, -1, g0[2])], {}, "-2", "group 0: outer and inner"),
                                        (c.forms, [g0, (0, 1, [])], {}, "-2", "group 1: nclause = 0"),
                                        (c.forms, [(0, 1, [g0[2][0], []])], {}, "-2", "group 0, clause 1 has 0 members"),
                                        (c.forms, [(0, 1, [g0[2][0] * 5])], {}, "-2", "group 0, clause 0 brings the group to 20 members"),
                                        (c.forms, [(0, 1, [g0[2][0] * 2, g0[2][0] * 2, [m0]])], {}, "-2", "group 0, clause 2 brings the group to 17 members"),
                                        (c.forms, [(0, 1, [g0[2][0] * 3])] * 3, {}, "-2", "group 2, clause 0 brings the members of all groups to 36"),
                                        (c.forms, [g0] * 5, {}, "-2", "ngroup"),
                                        (c.forms, [(0, 1, [[m0, (13, 0.0, -1)]])], {}, "-2", "group 0, clause 0, member 1 names form 13"),
                                        (c.forms, [(0, 1, [[(-1, 0.0, -1)]])], {}, "-2", "member 0 names form -1"),
                                        (c.forms, [(0, 1, [[(3, 0.0, 3)]])], {}, "-2", "group 0, clause 0, member 0: pc"),
                                        (c.forms[3:7], [(0, 1, [[(0, 0.0, 0)]])], dict(fprm=None), "-2", "member 0: pc"),
                                        (c.forms, [(0, 1, [[(3, float("nan"), -1)]])], {}, "-2", "member 0: c must be finite"),
                                        (c.forms, [(0, 1, [[(3, float("inf"), -1)]])], {}, "-2", "c must be finite"),
                                        ([[t0._replace(u=9)]], [mo.single_member()], {}, "-2", "form 0, term 0: u = 9"),
                                        ([[t0._replace(w=float("inf"))]], [mo.single_member()], {}, "-2", "finite"),
                                        ([c.forms[3] * 5], [mo.single_member()], {}, "-2", "form 0 has 10 terms"),
                                        (many, [mo.single_member()], {}, "-2", "nform"),
                                        ([c.forms[3] * 4] * 6, [mo.single_member()], {}, "-2", "form 5 brings the terms of all forms to 48"),
                                        (c.forms, [g0], dict(tol=-1.0), "-2", "tol"),
                                        (c.forms, [g0], dict(max_depth=31), "-2", "max_depth"),
                                        (c.forms, [g0], dict(sides=0), "-2", "sides")):
        kw = dict(dict(tol=mo.TOL, fprm=f2), **kw)
        with pytest.raises(api.NtgError, match=rc) as e:
            case.plan.minmax(x2, forms, groups, **kw)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(api.NtgError) as e:      # (the binding's own check: the struct has room for 8 clauses)
        case.plan.minmax(x2, c.forms, [(0, 1, [g0[2][0]] * 9)], mo.TOL, fprm=f2)
    assert "nclause = 9" in str(e.value)
    L = api.lib()
    nt = (api.C.c_int * 1)(1)
    term = (api.FormTerm * 1)(api.FormTerm(0, -1, -1, -1, 1.0, 0.0, 0.0))
    grp = (api.MinmaxGroup * 1)(api.MinmaxGroup(0, 1, 1, 0, (api.C.c_int * 8)(1, 0, 0, 0, 0, 0, 0, 0)))
    mem = (api.MinmaxMember * 1)(api.MinmaxMember(0, -1, 0.0))
    lo = dev(np.zeros((2, 1)))
    viol = torch.zeros((2, 2), dtype=torch.float64, device="cuda:0")
    which = torch.zeros((2, 1, 2), dtype=torch.int32, device="cuda:0")
    raw = lambda g, m, lo_, up_, v, w=None: L.ntg_batch_minmax(case.plan.h, 2, x2.data_ptr(), 1, nt, term, 0, None, 1, g, m, 1e-6, 30, 3, lo_, up_, None, None, w, None, None, v, None, None)
    assert raw(None, mem, None, None, None, which.data_ptr()) == -2 and "groups and members" in L.ntg_last_error().decode()
    assert raw(grp, None, None, None, None, which.data_ptr()) == -2 and "groups and members" in L.ntg_last_error().decode()
    assert raw(grp, mem, None, None, viol.data_ptr()) == -2 and "bounds" in L.ntg_last_error().decode()     # violation outputs without bounds
    assert raw(grp, mem, lo.data_ptr(), None, viol.data_ptr()) == -2 and raw(grp, mem, lo.data_ptr(), lo.data_ptr(), viol.data_ptr()) == 0
    assert raw(grp, mem, None, None, None) == -2 and "no output" in L.ntg_last_error().decode()
    assert raw(grp, mem, None, None, None, which.data_ptr()) == 0                                           # which alone is an output
    torch.cuda.synchronize()
    assert (which.cpu().numpy() == 0).all()
    mem0 = (api.MinmaxMember * 1)(api.MinmaxMember(0, 0, 0.0))                                              # pc named while d_fprm is null
    assert L.ntg_batch_minmax(case.plan.h, 2, x2.data_ptr(), 1, nt, term, 1, None, 1, grp, mem0, 1e-6, 30, 3, None, None, None, None, which.data_ptr(), None, None, None, None, None) == -2
    assert "group 0, clause 0, member 0 names a parameter, but d_fprm is null" in L.ntg_last_error().decode()
    host = api.Plan(dataclasses.replace(case.spec, family=-1), 0)   # NTG_FAM_HOST
    with pytest.raises(api.NtgError, match="-4") as e:
        host.minmax(x2, c.forms, [g0], mo.TOL, fprm=f2)
    assert "host-callback" in str(e.value)
    t3 = cf.config_T(nout=3, order=5, ninterv=4)   # outputs 0, 1 in one basis class, output 2 in another
    p3 = api.Plan(t3, 0)
    forms3, groups3 = mo.cross_class_declaration(t3)
    with pytest.raises(api.NtgError, match="-4") as e:
        p3.minmax(dev(np.zeros((2, t3.nC))), forms3, [mo.single_member(0)] + groups3, mo.TOL)
    assert "group 1 names forms 0 and 1 on outputs 0 and 2 of different basis classes" in str(e.value)
    assert set(cpu(p3.minmax(dev(np.zeros((2, t3.nC))), forms3, [mo.single_member(0), mo.single_member(1)], mo.TOL))) == set(KEYSW)   # different groups may use different classes
    pp = get_case("MPP")
    with pytest.raises(api.NtgError, match="-2") as e:      # a batch other than the grids'
        pp.plan.minmax(dev(pp.c.x[:5]), pp.c.forms, pp.c.groups, mo.TOL)
    assert "per-problem grids" in str(e.value)
    # 16 quadratic members on a long grid: 3025 + 250 (36 + 2) + 1 doubles of tables and 64 (16 * 11 + 1) of one wave's list are over 158 KiB
    big = api.Plan(cf._kincar_spec(1, 6, 3, 250, 251, 5.0, "kincar-l250"), 0)
    df, dg = mm.discs(big.spec, 0, 1, [(float(i), 0.0, 1.0) for i in range(16)])
    with pytest.raises(api.NtgError, match="-4") as e:
        big.minmax(dev(np.zeros((2, big.spec.nC))), df, [dg], mo.TOL)
    assert "LDS" in str(e.value)
    assert set(cpu(big.minmax(dev(np.zeros((2, big.spec.nC))), df[:8], [(dg[0], dg[1], [dg[2][0][:8]])], mo.TOL))) == set(KEYSW)   # ... and 8 of them fit
