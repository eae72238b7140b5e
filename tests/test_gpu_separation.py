"""-m gpu: ntg_batch_separation / Plan.separation -- the closest approach of pairs of planned bodies over the horizon, by bisection.

References: tests/separation_oracle.py (the definition in float64; its margins to the limits and its enclosure of the exact minimum are
checked in tests/test_separation_oracle.py), the library's own ntg_batch_extrema on the numpy differences (bit for bit: the kernel is
pinned to sos_poly and the level loop of extrema.hpp, not to a restatement of them) and Plan.interp (witness times and soundness).  Slack:
the header's rounding statement.  tol: one figure per case, max(1e-9 max |polygon point|, 64 slack).  Shapes are small: 4 / 8 / 20 knot
intervals (80 once, for the second pass over the intervals), 10 to 201 pairs."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import extrema_oracle as xo
import separation_oracle as po
from ntg_amd import api, configs as cf, family
from cert_common import NSAMP, cpu
from gpu_common import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("min", "when", "status", "npieces")
IDS = [f"{n}-d{d}" for n, d in po.CASES]


class Case:
    def __init__(self, name, deriv):
        self.c = c = po.inputs(name, deriv)
        self.name, self.npairs = f"{name} deriv {deriv}", len(c.pairs)
        self.plan = api.Plan(c.spec, 0)
        self.xd, self.pd = dev(c.x), dev(c.pairs, torch.int32)
        self._runs = {}

    def run(self, sep=None):
        """the whole case at its tolerance, without or with the threshold (computed once and kept)"""
        if sep not in self._runs:
            sd = None if sep is None else dev(np.full(self.npairs, sep))
            self._runs[sep] = cpu(self.plan.separation(self.xd, self.pd, self.c.bodies, self.c.deriv, tol=self.c.tol, sep=sd))
        return self._runs[sep]

    def sqdist(self, t):
        """the squared distance of every pair at the times t [ntimes] through Plan.interp: [npairs, ntimes]"""
        c = self.c
        z = self.plan.interp(self.xd, dev(np.ascontiguousarray(t)))
        torch.cuda.synchronize()
        z = z.cpu().numpy()
        iz = np.concatenate([[0], np.cumsum(c.spec.maxderiv)])
        out = np.zeros((self.npairs, len(t)))
        for q, (a, b, ga, gb) in enumerate(c.pairs):
            for oa, ob in zip(c.bodies[ga], c.bodies[gb]):
                out[q] += (z[a, :, iz[oa] + c.deriv] - z[b, :, iz[ob] + c.deriv]) ** 2
        return out


_cases = {}


def get_case(name, deriv=0):
    if (name, deriv) not in _cases:
        _cases[(name, deriv)] = Case(name, deriv)
    return _cases[(name, deriv)]


@pytest.fixture(scope="module", params=po.CASES, ids=IDS)
def case(request):
    return get_case(*request.param)


def same_as_oracle(got, ref, sl, tol, s2, label):
    """status and npieces equal; min, when and viol within the slack; the statement of a pair that ends OK"""
    assert got["status"].tolist() == [r["status"] for r in ref], label
    assert got["npieces"].tolist() == [r["npieces"] for r in ref], label
    rmin, rwhen = np.array([r["min"] for r in ref]), np.array([r["when"] for r in ref])
    err = max(float((np.abs(got["min"] - rmin) / sl[:, None]).max()), float((np.abs(got["when"] - rwhen) / sl).max()))
    if "viol" in got:
        rv = np.array([po.violation(r["min"], s2) for r in ref])
        err = max(err, float((np.abs(got["viol"] - rv) / sl[:, None]).max()))
        assert (got["viol"][:, 1] >= got["viol"][:, 0]).all()
    print(f"{label}: min, when and viol differ from the oracle's by at most {err:.3g} slack; {got['npieces'].mean():.1f} polygons per pair")
    assert err <= 1.0, label
    ok = got["status"] == po.OK
    assert (got["min"][ok, 0] >= np.minimum(got["min"][ok, 1] - tol, s2)).all(), label


# ---------------- 1. against the oracle ----------------
@pytest.mark.parametrize("thr", [False, True], ids=["nosep", "sep"])
def test_against_the_oracle(case, thr):
    c = case.c
    s2 = c.sep ** 2 if thr else np.inf
    got, ref = case.run(c.sep if thr else None), c.levels(s2)
    assert set(got) == set(KEYS + (("viol",) if thr else ()))
    same_as_oracle(got, ref, c.sl, c.tol, s2, f"{case.name}, sep {c.sep if thr else None}")
    assert (got["status"] == po.OK).all()
    if thr and c.name == "S4":
        at0 = np.array([r["depth"] == 0 for r in ref])
        assert at0.sum() == 85 and (got["npieces"][at0] == 4).all() and (got["npieces"][~at0] > 4).all()
        assert (got["viol"][:, 0] > 0).sum() == 110


# ---------------- 2. bit for bit against code that exists today ----------------
@pytest.mark.parametrize("name,deriv", [("S4", 0), ("S20", 0), ("Q8", 1)])
def test_bit_for_bit_the_extrema_of_the_differences(name, deriv):
    case = get_case(name, deriv)
    c, got = case.c, case.run()
    n = c.dl.shape[2]
    if c.name == "Q8":   # speed^2 = x'^2 + y'^2 + z'^2 is row 1 of the quadrotor plan; the yaw is not named
        plan, row = api.Plan(cf.config_D(ninterv=8), 0), 1
        x2 = np.concatenate([c.dl.reshape(case.npairs, -1), np.zeros((case.npairs, n))], axis=1)
    else:                # (x - cx)^2 + (y - cy)^2 with the centre at the origin
        plan, row = api.Plan(cf.config_OF(1, ninterv=c.spec.kninterv[0]), 0), 0
        plan.set_params(dev(np.zeros((case.npairs, 2))))
        x2 = c.dl.reshape(case.npairs, -1)
    ref = cpu(plan.extrema(dev(x2), c.tol, sides=1))
    assert np.array_equal(got["min"], ref["ext"][:, row, :2])
    assert np.array_equal(got["when"], ref["when"][:, row, 0])
    assert np.array_equal(got["status"], ref["status"][:, row]) and np.array_equal(got["npieces"], ref["npieces"][:, row])


# ---------------- 3. the witness time, and samples ----------------
def test_witness_and_samples(case):
    c, got = case.c, case.run()
    at = case.sqdist(got["when"])[np.arange(case.npairs), np.arange(case.npairs)]
    err = float((np.abs(at - got["min"][:, 1]) / c.sl).max())
    kn = np.asarray(c.kn(), dtype=np.float64)
    assert (got["when"] >= kn[0]).all() and (got["when"] <= kn[-1]).all()
    u = np.linspace(0.0, 1.0, NSAMP)
    t = kn[:-1, None] + (kn[1:] - kn[:-1])[:, None] * u[None, :]
    t[:, -1] = kn[1:]
    d2 = case.sqdist(np.clip(t, kn[0], kn[-1]).reshape(-1))
    below = float(((got["min"][:, 0, None] - d2) / c.sl[:, None]).max())
    print(f"{case.name}: the squared distance at the witness time differs from min_hi by at most {err:.3g} slack; samples below min_lo by at most {below:.3g} slack")
    assert err <= 1.0 and below <= 1.0
    assert (got["min"][:, 1] <= d2.min(axis=1) + c.sl).all()   # the attained value is no worse than what the samples see


# ---------------- 4. more intervals than lanes; an early stop ----------------
def test_more_intervals_than_lanes():
    """80 knot intervals: level 0 takes two passes over the intervals"""
    spec = cf._kincar_spec(1, 6, 3, 80, 401, 5.0, "kincar-2out-k6-l80")
    rng = np.random.default_rng(85)
    gv = xo.greville(spec)
    x = np.concatenate([8.0 * gv + rng.standard_normal((2, gv.size)), np.array([[0.0], [3.0]]) + rng.standard_normal((2, gv.size))], axis=1)
    bodies, pairs = np.array([[0, 1]], dtype=np.int32), np.array([[0, 1, 0, 0]], dtype=np.int32)
    polys = po.pair_polygons(spec, po.deltas(spec, x, bodies, pairs), 0, 0)
    sl = po.slack(spec, x, bodies, pairs, 0)
    tol = max(1e-9 * float(np.abs(polys).max()), 64.0 * float(sl.max()))
    plan = api.Plan(spec, 0)
    for sep in (None, 0.5):   # (the pair comes as close as 0.76)
        s2 = np.inf if sep is None else sep * sep
        ref = po.level_sep(polys[0], spec.knots[0], tol, s2)
        assert ref["status"] == po.OK and ref["depth"] <= 24 and ref["max_open"] <= 32   # far from the limits
        assert ref["npieces"] > 80 if sep is None else ref["npieces"] < 126 and ref["min"][0] >= s2
        got = cpu(plan.separation(dev(x), dev(pairs, torch.int32), bodies, tol=tol, sep=None if sep is None else dev(np.full(1, sep))))
        same_as_oracle(got, [ref], sl, tol, s2, f"80 intervals, sep {sep}")


def test_max_depth_stops_early_with_a_sound_enclosure():
    case = get_case("S4")
    c, full = case.c, case.run()
    got = cpu(case.plan.separation(case.xd, case.pd, c.bodies, c.deriv, tol=c.tol, max_depth=2))
    ref = c.levels(np.inf, 2)
    same_as_oracle(got, ref, c.sl, c.tol, np.inf, "S4, max_depth 2")
    assert (got["status"] == po.DEPTH).sum() > 100 and (got["status"] == po.OK).any()
    assert (got["min"][:, 0] <= full["min"][:, 1] + c.sl).all() and (full["min"][:, 0] <= got["min"][:, 1] + c.sl).all()
    for q in [q for q, r in enumerate(ref) if r["status"] == po.DEPTH][:3]:
        elo, ehi = po.exact_min(c.spec, c.dl[q], 0, 0, c.sl[q] / 8)
        assert got["status"][q] == po.DEPTH and got["min"][q, 0] - c.sl[q] <= ehi and elo <= got["min"][q, 1] + c.sl[q]


# ---------------- 5. independence and repeatability ----------------
def test_a_pair_alone_and_the_same_call_twice():
    case = get_case("S4")
    c = case.c
    sd = dev(np.full(case.npairs, c.sep))
    a = case.run(c.sep)
    b = cpu(case.plan.separation(case.xd, case.pd, c.bodies, c.deriv, tol=c.tol, sep=sd))
    q = 103   # (34, 40, 0, 2): two problems
    assert c.pairs[q, 0] != c.pairs[q, 1]
    one = cpu(case.plan.separation(case.xd, case.pd[q:q + 1].contiguous(), c.bodies, c.deriv, tol=c.tol, sep=sd[q:q + 1].contiguous()))
    for k in KEYS + ("viol",):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(one[k][0], a[k][q], equal_nan=True), k


# ---------------- 6. bad pairs ----------------
def test_bad_pairs_are_marked_and_read_nothing():
    """indices one past the ends, between good pairs"""
    case = get_case("S4")
    c = case.c
    ref = case.run(c.sep)
    nb = c.x.shape[0]
    good = [0, 50, 100, 200]
    pairs = np.array([c.pairs[good[0]], (-1, 0, 0, 0), c.pairs[good[1]], (0, nb, 0, 0), c.pairs[good[2]], (0, 0, 3, 0), c.pairs[good[3]]], dtype=np.int32)
    got = cpu(case.plan.separation(case.xd, dev(pairs, torch.int32), c.bodies, c.deriv, tol=c.tol, sep=dev(np.full(len(pairs), c.sep))))
    bad = np.array([1, 3, 5])
    assert (got["status"][bad] == api.SEP_BADPAIR).all() and (got["npieces"][bad] == 0).all()
    assert np.isnan(got["min"][bad]).all() and np.isnan(got["when"][bad]).all() and np.isnan(got["viol"][bad]).all()
    for k in KEYS + ("viol",):
        assert np.array_equal(got[k][::2], ref[k][good]), k


# ---------------- 7. refusals ----------------
def test_refusals():
    case = get_case("S4")
    c = case.c
    L = api.lib()
    ptr = lambda t: None if t is None else t.data_ptr()
    body = np.ascontiguousarray(c.bodies)
    npairs = 4
    mn = torch.full((npairs, 2), -7.0, dtype=torch.float64, device="cuda:0")
    viol = torch.full((npairs, 2), -7.0, dtype=torch.float64, device="cuda:0")
    sep = dev(np.full(npairs, 2.0))

    def raw(batch=c.x.shape[0], x=case.xd, nbody=3, ndim=2, bo=body, deriv=0, npairs=npairs, pairs=case.pd, sep=None, tol=1e-9, depth=30, m=mn, v=None):
        rc = L.ntg_batch_separation(case.plan.h, batch, ptr(x), nbody, ndim, None if bo is None else bo.ctypes.data_as(api.ip), deriv, npairs, ptr(pairs), ptr(sep), tol, depth,
                                    ptr(m), None, None, None, ptr(v), None)
        return rc, L.ntg_last_error().decode()

    for kw, word in ((dict(ndim=0), "ndim"), (dict(ndim=5), "ndim"), (dict(nbody=0), "nbody"), (dict(nbody=17), "nbody"), (dict(deriv=-1), "deriv"), (dict(deriv=3), "deriv"),
                     (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"), (dict(depth=-1), "max_depth"), (dict(depth=31), "max_depth"),
                     (dict(x=None), "null"), (dict(bo=None), "null"), (dict(pairs=None), "null"), (dict(m=None), "no output"), (dict(v=viol), "d_sep"),
                     (dict(bo=np.array([[0, 1], [2, 3], [4, 6]], dtype=np.int32)), "output 6")):
        rc, msg = raw(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    assert raw(npairs=0, depth=31)[0] == -2 and raw(batch=0, m=None)[0] == -2   # the arguments before the empty call's 0
    assert raw(npairs=0, sep=sep, v=viol)[0] == 0 and raw(batch=0, sep=sep, v=viol)[0] == 0
    torch.cuda.synchronize()
    assert (mn == -7.0).all() and (viol == -7.0).all()   # nothing written
    assert raw(sep=sep, v=viol)[0] == 0
    torch.cuda.synchronize()
    assert (mn != -7.0).all() and (viol != -7.0).all()
    tp = api.Plan(cf.config_T(), 0)   # output 2 has a basis class of its own
    pd = dev(np.array([[0, 1, 0, 0]]), torch.int32)
    with pytest.raises(api.NtgError, match="-4") as e:
        tp.separation(dev(np.zeros((2, tp.spec.nC))), pd, [[0, 2]])
    assert "outputs 0 and 2" in str(e.value)
    assert set(cpu(tp.separation(dev(np.zeros((2, tp.spec.nC))), pd, [[0, 1]]))) == set(KEYS)
    g = xo.inputs("G4")                # per-problem grids in force
    gp = api.Plan(g.spec, 0)
    gp.set_grids(dev(g.knots), dev(g.bps), with_precond=False)
    with pytest.raises(api.NtgError, match="-4") as e:
        gp.separation(dev(g.x), dev(np.array([[0, 0, 0, 0]]), torch.int32), [[0, 1]])
    assert "per-problem grids" in str(e.value)
    hp = api.Plan(dataclasses.replace(xo.rows_spec(), family=-1), 0)   # host-callback plans
    with pytest.raises(api.NtgError, match="-4"):
        hp.separation(dev(np.zeros((2, hp.spec.nC))), pd, [[0, 1]])
    bs = cf._kincar_spec(1, 6, 3, 300, 301, 5.0, "kincar-l300")   # 385 + 300 (36 + 2) + 1 doubles of tables and 4 (1806 + 768) of the waves: 172 KiB
    with pytest.raises(api.NtgError, match="-4") as e:
        api.Plan(bs, 0).separation(dev(np.zeros((2, bs.nC))), pd, [[0, 1]])
    assert "LDS" in str(e.value)


# ---------------- 8. a module family ----------------
def test_a_module_family_plan_is_certified_like_a_built_in_one():
    spec = xo.testfam_spec()   # three outputs in one basis class
    x = xo.inputs("T3").x
    bodies = np.array([[0], [1], [2]], dtype=np.int32)
    pairs = np.array([(0, 1, 0, 0), (0, 0, 0, 1), (1, 2, 2, 1), (2, 0, 1, 1)], dtype=np.int32)
    polys = po.pair_polygons(spec, po.deltas(spec, x, bodies, pairs), 0, 0)
    sl = po.slack(spec, x, bodies, pairs, 0)
    tol = max(1e-9 * float(np.abs(polys).max()), 64.0 * float(sl.max()))
    ref = [po.level_sep(P, spec.knots[0], tol) for P in polys]
    assert all(r["status"] == po.OK and r["depth"] <= 24 and r["max_open"] <= 32 for r in ref)
    fam = api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "testfam_module.hip")))
    mp, bp = api.Plan(dataclasses.replace(spec, family=fam), 0), api.Plan(spec, 0)
    got = cpu(mp.separation(dev(x), dev(pairs, torch.int32), bodies, tol=tol))
    own = cpu(bp.separation(dev(x), dev(pairs, torch.int32), bodies, tol=tol))
    same_as_oracle(got, ref, sl, tol, np.inf, "testfam module, one coordinate per body")
    for k in KEYS:
        assert np.array_equal(got[k], own[k]), k
