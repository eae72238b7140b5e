"""-m gpu: ntg_batch_envelope_sos / Plan.envelope_sos -- bounds of the sum-of-squares trajectory rows over whole pieces of time.

Reference: tests/envelope_sos_oracle.py, the definition of include/ntg_amd.h in exact rational arithmetic by another route (de Boor's
recursion on polynomials, the power basis, one conversion to Bernstein form at the end), and the library's own callbacks through
Plan.check for soundness -- which is also what audits every family's declaration against its nltcf.  Tolerance everywhere: sos_slack =
2^-40 sum_t S_t^2, the header's rounding statement.  Shapes are small: 4 / 5 / 8 and 20 knot intervals, batches 1 to 67.
"""
import dataclasses

import numpy as np
import pytest
import torch

import envelope_oracle as eo
import envelope_sos_oracle as so
from ntg_amd import api, configs as cf
from cert_common import NSAMP, cpu, field_x, greville, obstacle_x, piece_times, scaled_grids, within
from gpu_common import dev

pytestmark = pytest.mark.gpu
NBIG = 67   # leaves the persistent loop a partial last pass


# ---------------- the plans of tests 1 and 2 ----------------
class Case:
    """a plan, NBIG problems on it (coefficients, bounds, parameters) and the number of them the exact oracle is run on"""

    def __init__(self, name, spec, x, lower, upper, prm, noracle, nsubs):
        self.name, self.spec, self.x, self.lower, self.upper, self.prm, self.noracle, self.nsubs = name, spec, x, lower, upper, prm, noracle, nsubs
        self.plan = api.Plan(spec, 0)
        self._oracle = {}

    def sub(self, sl):
        """set the parameters of problems sl (families that take them) and return their device tensors x, lower, upper"""
        if self.prm is not None:
            self.plan.set_params(dev(self.prm[sl]))
        return dev(self.x[sl]), dev(self.lower[sl]), dev(self.upper[sl])

    def params(self, sl):
        return None if self.prm is None else self.prm[sl]

    def oracle(self, nsub):
        if nsub not in self._oracle:
            sl = slice(0, self.noracle)
            self._oracle[nsub] = so.row_envelope(self.spec, self.x[sl], nsub, self.params(sl))
        return self._oracle[nsub]

    def slack(self, sl):
        return so.sos_slack(self.spec, self.x[sl], self.params(sl))


def make_case(name):
    if name in ("O4", "O20"):
        spec = cf.config_O(ninterv=4) if name == "O4" else cf.config_O()
        lo, up = cf.obstacle_bounds(NBIG)
        return Case(name, spec, obstacle_x(spec, NBIG, 41), lo, up, None, 5, (0, 2))
    if name == "OF5":
        spec = cf.config_OF(3, ninterv=5)
        prm, lo, up = cf.obstacle_field_problems(NBIG, 3)
        return Case(name, spec, field_x(spec, lo, 42), lo, up, prm, 5, (1,))
    spec = cf.config_D(ninterv=8)   # order 8: the KM = 10 instance, products of degree 10 (thrust^2) and 12 (speed^2)
    lo, up = cf.quadrotor_bounds(NBIG)
    return Case(name, spec, np.random.default_rng(43).standard_normal((NBIG, spec.nC)), lo, up, None, 3, (0, 1))


CASES = ["O4", "O20", "OF5", "D8"]
_cases = {}


@pytest.fixture(scope="module", params=CASES)
def case(request):
    if request.param not in _cases:
        _cases[request.param] = make_case(request.param)
    return _cases[request.param]


def get_case(name):
    if name not in _cases:
        _cases[name] = make_case(name)
    return _cases[name]


# ---------------- 1. oracle agreement ----------------
def test_rows_match_the_exact_oracle(case):
    sl = slice(0, case.noracle)
    assert case.plan.sos_rows().tolist() == so.flags(case.spec).tolist() == [1] * case.spec.nnltc
    xd, _, _ = case.sub(sl)
    for nsub in case.nsubs:
        got = cpu(case.plan.envelope_sos(xd, nsub))
        assert set(got) == {"q_lo", "q_hi"} and got["q_lo"].shape == (case.noracle, case.spec.nnltc, max(case.spec.kninterv) << nsub)
        olo, ohi = case.oracle(nsub)
        s = case.slack(sl)[:, :, None]
        within(got["q_lo"], olo, s, f"{case.name} nsub {nsub} q_lo"); within(got["q_hi"], ohi, s, f"{case.name} nsub {nsub} q_hi")


# ---------------- 2. soundness against the library's own callbacks ----------------
@pytest.mark.parametrize("nb", [1, 5, NBIG])
def test_rows_enclose_check(case, nb):
    spec, nsub = case.spec, 1
    sl = slice(0, nb)
    xd, lo, up = case.sub(sl)
    got = cpu(case.plan.envelope_sos(xd, nsub))
    t = piece_times(api.envelope_pieces(spec, 0, nsub))
    chk = cpu(case.plan.check(xd, lo, up, dev(t.reshape(-1)), want_rows=True))
    rows = chk["rows"][:, spec.nltc:].reshape(nb, spec.nnltc, t.shape[0], NSAMP)
    s = case.slack(sl)[:, :, None, None]
    below, above = (got["q_lo"][..., None] - rows) / s, (rows - got["q_hi"][..., None]) / s
    worst = float(max(below.max(), above.max()))
    print(f"{case.name} batch {nb}: the family's rows outside the bounds by at most {worst:.3g} slack")
    assert worst <= 1.0
    if nb == NBIG:   # a problem's figures do not depend on the batch around it
        xd2, _, _ = case.sub(slice(2, 4))
        two = cpu(case.plan.envelope_sos(xd2, nsub))
        assert np.array_equal(two["q_lo"], got["q_lo"][2:4]) and np.array_equal(two["q_hi"], got["q_hi"][2:4])


# ---------------- 3. known answer ----------------
def test_known_answer():
    """x(t) = 8 t, y = 0.5 + delta: the row is (8 t - 20)^2 + delta^2, closest to the obstacle at the knot t = 2.5"""
    spec = cf.config_O()
    p = get_case("O20").plan
    delta, gv = 1.25, greville(spec)
    x = np.concatenate([8.0 * gv, np.full(gv.size, 0.5 + delta)])[None, :]
    s = so.sos_slack(spec, x)[0, 0]
    for nsub in range(5):
        lo, up = cf.obstacle_bounds(1, radius=3.0)
        got = cpu(p.envelope_sos(dev(x), nsub, dev(lo), dev(up)))
        print(f"nsub {nsub}: viol {got['viol'][0]!r} where {got['where'][0]}, slack {s:.3g}")
        assert abs(got["viol"][0] - (9.0 - delta * delta)) <= s
        assert got["where"][0, 0] == 0 and got["where"][0, 1] in ((10 << nsub) - 1, 10 << nsub)
        lo, up = cf.obstacle_bounds(1, radius=1.0)
        got = cpu(p.envelope_sos(dev(x), nsub, dev(lo), dev(up)))
        assert got["viol"][0] == 0.0 and tuple(got["where"][0]) == (-1, -1)


# ---------------- 4. nesting ----------------
def test_finer_pieces_certify_no_less():
    c = get_case("O20")
    spec, nb = c.spec, 5
    xd, lo, up = c.sub(slice(0, nb))
    s = c.slack(slice(0, nb))[:, 0]
    viol = [cpu(c.plan.envelope_sos(xd, nsub, lo, up))["viol"] for nsub in range(5)]
    t = piece_times(api.envelope_pieces(spec, 0, 4))
    sampled = cpu(c.plan.check(xd, lo, up, dev(t.reshape(-1))))["viol"]
    print("certified", np.array(viol), "sampled", sampled)
    assert (sampled > 0).any()
    for nsub in range(4):   # the polygons of the sub-pieces lie in the hull of the parent's
        assert (viol[nsub + 1] <= viol[nsub] + s).all(), nsub
    for nsub in range(5):
        assert (viol[nsub] >= sampled - s).all(), nsub


# ---------------- 5. two-sided bounds ----------------
def test_violation_is_the_maximum_over_the_returned_bounds():
    """the reduction alone: viol / where against the maximum recomputed from the q_lo / q_hi the same call returned, tie rule included"""
    c = get_case("D8")
    scale = np.array([1e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0, 1.0])   # from a hover (no violation) to flights that break both limits
    nb = len(scale)
    x = c.x[:nb] * scale[:, None]
    for nsub in (0, 1):
        got = cpu(c.plan.envelope_sos(dev(x), nsub, dev(c.lower[:nb]), dev(c.upper[:nb])))
        viol, where = so.violation(c.spec, got["q_lo"], got["q_hi"], c.lower[:nb], c.upper[:nb])
        print("nsub", nsub, "viol", got["viol"], "where", got["where"].tolist())
        assert (viol > 0).any()
        assert np.array_equal(got["viol"], viol) and np.array_equal(got["where"], where)


# ---------------- 6. per-problem grids ----------------
def test_per_problem_grids():
    spec, nsub = cf.config_O(ninterv=4), 1
    scales = np.array([0.5, 1.0, 1.7, 2.0, 3.0])
    nb = len(scales)
    knots, bps = scaled_grids(spec, scales)
    x = obstacle_x(spec, nb, 61)
    x[:, :spec.ncoef[0]] *= scales[:, None]   # x = 8 t on the problem's own horizon
    lo, up = cf.obstacle_bounds(nb)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    xd = dev(x)
    got = cpu(p.envelope_sos(xd, nsub, dev(lo), dev(up)))
    olo, ohi = so.row_envelope(spec, x, nsub, knots=knots)
    s = so.sos_slack(spec, x, knots=knots)
    within(got["q_lo"], olo, s[:, :, None], "grids q_lo"); within(got["q_hi"], ohi, s[:, :, None], "grids q_hi")
    oviol, owhere = so.violation(spec, olo, ohi, lo, up)
    assert (np.abs(got["viol"] - oviol) <= s[:, 0]).all()
    t = np.stack([piece_times(api.envelope_pieces(knots[b], nsub=nsub)).reshape(-1) for b in range(nb)])
    chk = cpu(p.check(xd, dev(lo), dev(up), dev(t), want_rows=True))
    rows = chk["rows"][:, spec.nltc:].reshape(nb, 1, -1, NSAMP)
    below, above = (got["q_lo"][..., None] - rows) / s[:, :, None, None], (rows - got["q_hi"][..., None]) / s[:, :, None, None]
    print(f"grids: the family's rows outside the bounds by at most {float(max(below.max(), above.max())):.3g} slack")
    assert max(below.max(), above.max()) <= 1.0
    with pytest.raises(api.NtgError, match="-2"):   # the grids are for exactly this batch
        p.envelope_sos(xd[:3].contiguous(), nsub)


# ---------------- 7. flags and refusals ----------------
def test_mixed_basis_classes():
    tspec = cf.config_T()   # row 0 names output 0 (order 5, 4 intervals) and output 2 (order 6, 5 intervals)
    tp = api.Plan(tspec, 0)
    assert tp.sos_rows().tolist() == [0, 0]
    x = dev(np.random.default_rng(2).standard_normal((2, tspec.nC)))
    with pytest.raises(api.NtgError, match="-4") as e:
        tp.envelope_sos(x, 0)
    assert "declares none" in str(e.value)


def test_partial_certificate():
    t0 = cf.config_T()
    spec = dataclasses.replace(t0, order=[t0.order[0]] * 3, kninterv=[t0.kninterv[0]] * 3, knots=[np.array(t0.knots[0]) for _ in range(3)])
    assert so.flags(spec).tolist() == [1, 0]
    p = api.Plan(spec, 0)
    assert p.sos_rows().tolist() == [1, 0]
    nb, nsub = 3, 1
    x = np.random.default_rng(3).standard_normal((nb, spec.nC))
    got = cpu(p.envelope_sos(dev(x), nsub))
    olo, ohi = so.row_envelope(spec, x, nsub)
    assert np.isneginf(olo[:, 1]).all() and np.isposinf(ohi[:, 1]).all()
    s = so.sos_slack(spec, x)
    s[:, 1] = 1.0   # (no finite figure of row 1 is compared)
    within(got["q_lo"], olo, s[:, :, None], "testfam q_lo"); within(got["q_hi"], ohi, s[:, :, None], "testfam q_hi")
    b = dev(np.zeros((nb, spec.nbounds)))
    with pytest.raises(api.NtgError, match="-4") as e:
        p.envelope_sos(dev(x), nsub, b, b)
    assert "row 1" in str(e.value)


def test_refusals():
    mp = api.Plan(cf.config_E(ninterv=4, narms=2), 0)   # the manipulator's rows are sines
    assert mp.sos_rows().tolist() == [0, 0]
    with pytest.raises(api.NtgError, match="-4"):
        mp.envelope_sos(dev(np.zeros((2, mp.spec.nC))), 0)
    kp = api.Plan(cf._kincar_spec(1, 6, 3, 4, 21, 5.0, "kincar-l4"), 0)
    assert kp.sos_rows().shape == (0,)
    with pytest.raises(api.NtgError, match="-2") as e:
        kp.envelope_sos(dev(np.zeros((2, kp.spec.nC))), 0)
    assert "nnltc" in str(e.value)
    fp = api.Plan(cf.config_OF(3, ninterv=5), 0)        # the centres are parameters: not set yet
    with pytest.raises(api.NtgError, match="-2") as e:
        fp.envelope_sos(dev(np.zeros((2, fp.spec.nC))), 0)
    assert "ntg_plan_set_params" in str(e.value)
    c = get_case("O4")
    x = dev(c.x[:2])
    with pytest.raises(api.NtgError):
        c.plan.envelope_sos(x, 7)
    L = api.lib()
    q = torch.empty((2, 1, 4), dtype=torch.float64, device="cuda:0")
    ptr = lambda t: None if t is None else t.data_ptr()
    assert L.ntg_batch_envelope_sos(c.plan.h, 2, ptr(x), 7, None, None, ptr(q), None, None, None, None) == -2 and "nsub" in L.ntg_last_error().decode()
    assert L.ntg_batch_envelope_sos(c.plan.h, 0, ptr(x), 7, None, None, ptr(q), None, None, None, None) == -2   # nsub before the empty batch
    assert L.ntg_batch_envelope_sos(c.plan.h, 0, ptr(x), 0, None, None, ptr(q), None, None, None, None) == 0    # an empty batch
    assert L.ntg_batch_envelope_sos(c.plan.h, 2, None, 0, None, None, ptr(q), None, None, None, None) == -2     # null d_x
    assert L.ntg_batch_envelope_sos(c.plan.h, 2, ptr(x), 0, None, None, None, None, None, None, None) == -2     # all four outputs null
    v = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    assert L.ntg_batch_envelope_sos(c.plan.h, 2, ptr(x), 0, None, None, None, None, ptr(v), None, None) == -2 and "bounds" in L.ntg_last_error().decode()
    hp = api.Plan(dataclasses.replace(kp.spec, family=-1), 0)   # host-callback plans
    with pytest.raises(api.NtgError, match="-4"):
        hp.envelope_sos(x, 0)


def test_nan_stays_in_its_own_problem():
    c = get_case("O4")
    nb, nsub = 4, 1
    xd, lo, up = c.sub(slice(0, nb))
    clean = cpu(c.plan.envelope_sos(xd, nsub, lo, up))
    x = c.x[:nb].copy()
    x[2, 1] = np.nan   # a coefficient of x on the first knot interval
    got = cpu(c.plan.envelope_sos(dev(x), nsub, lo, up))
    for k in clean:
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
    assert np.isnan(got["q_lo"][2, 0, :2]).all() and np.isnan(got["q_hi"][2, 0, :2]).all()
    assert np.isnan(got["viol"][2]) and tuple(got["where"][2]) == (0, 0)


# ---------------- 8. repeatability ----------------
def test_two_calls_are_bit_equal(case):
    xd, lo, up = case.sub(slice(0, NBIG))
    a = cpu(case.plan.envelope_sos(xd, 1, lo, up))
    b = cpu(case.plan.envelope_sos(xd, 1, lo, up))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
