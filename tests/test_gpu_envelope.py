"""-m gpu: ntg_batch_envelope / Plan.envelope -- bounds of every flag entry and every linear trajectory row over whole pieces of time.

Reference: tests/envelope_oracle.py, the definition of include/ntg_amd.h restated in numpy / scipy by another route (scipy's BSpline and
a Bernstein collocation solve instead of the blossom), and the library's own point evaluations (Plan.interp, Plan.check) for soundness.
Tolerance everywhere: slack = 2^-42 max|c_o| (2 (k - 1) / h_min)^r for entry iz[o] + r, the header's rounding statement; for a row the
combination sum_v |ltc[i][v]| slack_v of its entries' slacks.  Shapes are small: 4 / 5 and 20 knot intervals, batches 1 to 67.
"""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

import envelope_oracle as eo
from ntg_amd import api, configs as cf
from cert_common import NSAMP, cpu, kincar_spec, piece_times, rows_spec, scaled_grids, within
from gpu_common import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def encloses(lo, hi, samples, sl, label):
    """lo, hi [nb, n, npc], samples [nb, n, npc, NSAMP], sl [nb, n]"""
    assert samples.shape == lo.shape + (NSAMP,) and sl.shape == lo.shape[:2]
    below, above = (lo[..., None] - samples) / sl[:, :, None, None], (samples - hi[..., None]) / sl[:, :, None, None]
    worst = float(max(below.max(), above.max()))
    print(f"{label}: samples outside the bounds by at most {worst:.3g} slack")
    assert worst <= 1.0, label


# ---------------- the plans ----------------
@pytest.fixture(scope="module")
def kplan():
    return api.Plan(kincar_spec(), 0)


@pytest.fixture(scope="module")
def rplan():
    return api.Plan(rows_spec(), 0)


@pytest.fixture(scope="module")
def rcase(rplan):
    """five problems of the rows plan at nsub = 1: coefficients, the oracle's envelopes, the kernel's"""
    spec, nb, nsub = rplan.spec, 5, 1
    x = np.random.default_rng(11).standard_normal((nb, spec.nC))
    olo, ohi = eo.row_envelope(spec, x, nsub)
    got = cpu(rplan.envelope(dev(x), nsub, want_rows=True))
    return dict(spec=spec, nb=nb, nsub=nsub, x=x, olo=olo, ohi=ohi, got=got, sl=eo.row_slack(spec, x))


# ---------------- entries ----------------
@pytest.mark.parametrize("nsub", [0, 2])
def test_entries_of_testfam_match_the_oracle(nsub):
    """three outputs, two basis classes (orders 5 and 6 on 4 and 5 intervals): the shorter outputs' last pieces are the empty set"""
    spec, nb = cf.config_T(), 5
    p = api.Plan(spec, 0)
    x = np.random.default_rng(1).standard_normal((nb, spec.nC))
    got = cpu(p.envelope(dev(x), nsub))
    npc = 5 << nsub
    assert got["lo"].shape == (nb, spec.nz, npc) and set(got) == {"lo", "hi"}
    olo, ohi = eo.entry_envelope(spec, x, nsub)
    sl = eo.slack(spec, x)[:, :, None]
    within(got["lo"], olo, sl, f"testfam nsub {nsub} lo"); within(got["hi"], ohi, sl, f"testfam nsub {nsub} hi")
    own = 4 << nsub
    assert np.isposinf(got["lo"][:, :6, own:]).all() and np.isneginf(got["hi"][:, :6, own:]).all()
    assert np.isfinite(got["lo"][:, 6:]).all() and np.isfinite(got["hi"][:, :6, :own]).all()


@pytest.mark.parametrize("nb", [1, 5, 67])
def test_entries_enclose_interp(kplan, nb):
    """soundness against the library's own point evaluation; 67 problems leave the persistent loop a partial last pass"""
    spec, nsub = kplan.spec, 1
    x = np.random.default_rng(20 + nb).standard_normal((nb, spec.nC))
    xd = dev(x)
    got = cpu(kplan.envelope(xd, nsub))
    t = piece_times(api.envelope_pieces(spec, 0, nsub))
    z = kplan.interp(xd, dev(t.reshape(-1))).cpu().numpy().reshape(nb, t.shape[0], NSAMP, spec.nz).transpose(0, 3, 1, 2)
    encloses(got["lo"], got["hi"], z, eo.slack(spec, x), f"kincar batch {nb}")
    if nb == 67:   # a problem's figures do not depend on the batch around it
        two = cpu(kplan.envelope(xd[2:4].contiguous(), nsub))
        assert np.array_equal(two["lo"], got["lo"][2:4]) and np.array_equal(two["hi"], got["hi"][2:4])
        again = cpu(kplan.envelope(xd, nsub))
        assert np.array_equal(again["lo"], got["lo"]) and np.array_equal(again["hi"], got["hi"])


def test_known_answers(kplan):
    spec, nsub = kplan.spec, 2
    n = spec.ncoef[0]
    # a constant spline: its constant bit for bit, zero derivatives
    c = 0.7
    got = cpu(kplan.envelope(dev(np.full((1, spec.nC), c)), nsub))
    for v in (0, 3):
        assert (got["lo"][0, v] == c).all() and (got["hi"][0, v] == c).all()
    for v in (1, 2, 4, 5):
        assert (got["lo"][0, v] == 0.0).all() and (got["hi"][0, v] == 0.0).all()
    # coefficients = the Greville abscissae: the spline is t
    t = eo.aug_knots(spec.knots[0], 6, 3)
    gv = np.array([t[i + 1:i + 6].mean() for i in range(n)])
    x = np.concatenate([gv, gv])[None, :]
    got = cpu(kplan.envelope(dev(x), nsub))
    ends = api.envelope_pieces(spec, 0, nsub)
    sl = eo.slack(spec, x)[0]
    for v in (0, 3):
        assert (np.abs(got["lo"][0, v] - ends[:-1]) <= sl[v]).all() and (np.abs(got["hi"][0, v] - ends[1:]) <= sl[v]).all()
        assert (np.abs(got["lo"][0, v + 1] - 1.0) <= sl[v + 1]).all() and (np.abs(got["hi"][0, v + 1] - 1.0) <= sl[v + 1]).all()


def test_nan_stays_in_its_own_problem(rplan):
    spec, nb, nsub = rplan.spec, 4, 1
    x = np.random.default_rng(31).standard_normal((nb, spec.nC))
    lower = np.full((nb, spec.nbounds), -1.0); upper = np.full((nb, spec.nbounds), 1.0)
    clean = cpu(rplan.envelope(dev(x), nsub, dev(lower), dev(upper), want_rows=True))
    x[2, 5] = np.nan   # a coefficient of x in the first two knot intervals
    got = cpu(rplan.envelope(dev(x), nsub, dev(lower), dev(upper), want_rows=True))
    for k in clean:
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
    assert np.isnan(got["lo"][2, 0, :4]).all() and np.isnan(got["hi"][2, 0, :4]).all() and np.isfinite(got["lo"][2, 0, 4:]).all()
    assert np.isfinite(got["lo"][2, 3:]).all()                                   # y is clean
    assert np.isnan(got["row_lo"][2, 1, :4]).all() and np.isfinite(got["row_lo"][2, 0]).all()
    assert np.isnan(got["viol"][2]) and tuple(got["where"][2]) == (1, 0)         # the first NaN by row * npc + piece


# ---------------- rows ----------------
def test_rows_match_the_oracle(rcase):
    g = rcase["got"]
    assert g["row_lo"].shape == (rcase["nb"], 3, 40) and set(g) == {"lo", "hi", "row_lo", "row_hi"}
    sl = rcase["sl"][:, :, None]
    within(g["row_lo"], rcase["olo"], sl, "rows lo"); within(g["row_hi"], rcase["ohi"], sl, "rows hi")
    # x' - y' + 0.5 y'': the row's own polygon, tighter than the sum of its entries' hulls
    wide = (g["hi"][:, 1] - g["lo"][:, 1]) + (g["hi"][:, 4] - g["lo"][:, 4]) + 0.5 * (g["hi"][:, 5] - g["lo"][:, 5])
    assert ((g["row_hi"] - g["row_lo"])[:, 2] < 0.9 * wide).any()


def test_rows_enclose_check_and_certify(rplan, rcase):
    spec, nb, nsub, x = rcase["spec"], rcase["nb"], rcase["nsub"], rcase["x"]
    g, olo, ohi, sl = rcase["got"], rcase["olo"], rcase["ohi"], rcase["sl"]
    xd = dev(x)
    t = piece_times(api.envelope_pieces(spec, 0, nsub))
    s0 = spec.nlic
    # bounds that most problems violate somewhere
    lower = np.zeros((nb, spec.nbounds)); upper = np.zeros((nb, spec.nbounds))
    mid = 0.5 * (olo.min(axis=2) + ohi.max(axis=2)); half = 0.25 * (ohi.max(axis=2) - olo.min(axis=2))
    lower[:, s0:s0 + 3] = mid - half; upper[:, s0:s0 + 3] = mid + half
    chk = cpu(rplan.check(xd, dev(lower), dev(upper), dev(t.reshape(-1)), want_rows=True))
    rows = chk["rows"].reshape(nb, 3, t.shape[0], NSAMP)
    encloses(g["row_lo"], g["row_hi"], rows, sl, "rows against check")
    env = cpu(rplan.envelope(xd, nsub, dev(lower), dev(upper), want_entries=False))
    assert set(env) == {"viol", "where"}
    oviol, owhere = eo.violation(spec, olo, ohi, lower, upper)
    print("certified violation", env["viol"], "sampled", chk["viol"])
    assert (chk["viol"] > 0).any()
    assert (env["viol"] >= chk["viol"] - sl.max(axis=1)).all()
    assert (np.abs(env["viol"] - oviol) <= sl.max(axis=1)).all()
    # bounds 1.0 outside the oracle's envelope: certified
    lower[:, s0:s0 + 3] = olo.min(axis=2) - 1.0; upper[:, s0:s0 + 3] = ohi.max(axis=2) + 1.0
    env = cpu(rplan.envelope(xd, nsub, dev(lower), dev(upper), want_entries=False))
    assert (env["viol"] == 0.0).all() and (env["where"] == -1).all()
    # ... and the upper bound of row 1 pulled 0.1 inside it on one problem
    b = 3
    upper[b, s0 + 1] = ohi[b, 1].max() - 0.1
    env = cpu(rplan.envelope(xd, nsub, dev(lower), dev(upper), want_entries=False))
    assert (np.delete(env["viol"], b) == 0.0).all() and (np.delete(env["where"], b, axis=0) == -1).all()
    assert abs(env["viol"][b] - 0.1) <= sl[b, 1] and tuple(env["where"][b]) == (1, int(np.argmax(ohi[b, 1])))
    # one-sided: an absent bound does not count
    lower[:, s0:s0 + 3] = -cf.INF_BOUND; upper[:, s0:s0 + 3] = cf.INF_BOUND
    env = cpu(rplan.envelope(xd, nsub, dev(lower), dev(upper), want_entries=False))
    assert (env["viol"] == 0.0).all()


def test_per_problem_grids(rcase):
    """five horizons scaled by 0.8 .. 1.3: every problem's figures equal, to slack, those of a plan built on that problem's own knots"""
    spec, nb, nsub, x = rcase["spec"], rcase["nb"], 1, rcase["x"]
    knots, bps = scaled_grids(spec, np.linspace(0.8, 1.3, nb))
    lower = np.full((nb, spec.nbounds), -2.0); upper = np.full((nb, spec.nbounds), 2.0)
    p = api.Plan(spec, 0)
    p.set_grids(dev(knots), dev(bps), with_precond=False)
    xd = dev(x)
    got = cpu(p.envelope(xd, nsub, dev(lower), dev(upper), want_rows=True))
    assert (got["viol"] > 0).any()
    with pytest.raises(api.NtgError, match="-2"):   # the grids are for exactly this batch
        p.envelope(xd[:3].contiguous(), nsub)
    p.clear_grids()
    for b in range(nb):
        sb = dataclasses.replace(spec, knots=[knots[b].copy() for _ in range(spec.nout)], bps=bps[b].copy())
        own = cpu(api.Plan(sb, 0).envelope(xd[b:b + 1].contiguous(), nsub, dev(lower[b:b + 1]), dev(upper[b:b + 1]), want_rows=True))
        sl = eo.slack(sb, x[b:b + 1])[0][:, None]; rs = eo.row_slack(sb, x[b:b + 1])[0][:, None]
        for k, s in (("lo", sl), ("hi", sl), ("row_lo", rs), ("row_hi", rs)):
            assert (np.abs(got[k][b] - own[k][0]) <= s).all(), (b, k)
        assert abs(got["viol"][b] - own["viol"][0]) <= rs.max() and np.array_equal(got["where"][b], own["where"][0])
    # ... and the scaled grid changes the derivatives' bounds
    assert np.abs(got["lo"][0, 1] - got["lo"][nb - 1, 1]).max() > 1e-3


# ---------------- errors ----------------
def _raw(plan, nb, x, nsub, lower=None, upper=None, lo=None, hi=None, rlo=None, rhi=None, viol=None, where=None):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = api.lib().ntg_batch_envelope(plan.h, nb, ptr(x), nsub, ptr(lower), ptr(upper), ptr(lo), ptr(hi), ptr(rlo), ptr(rhi), ptr(viol), ptr(where), None)
    return rc, api.lib().ntg_last_error().decode()


def test_errors(kplan, rplan):
    spec, nb = kplan.spec, 2
    x = dev(np.ones((nb, spec.nC)))
    buf = torch.empty((nb, spec.nz, 20 << 6), dtype=torch.float64, device="cuda:0")
    with pytest.raises(api.NtgError):
        kplan.envelope(x, 7)
    rc, msg = _raw(kplan, nb, x, 7, lo=buf)
    assert rc == -2 and "nsub" in msg
    assert _raw(kplan, nb, x, -1, lo=buf)[0] == -2
    assert _raw(kplan, nb, None, 0, lo=buf)[0] == -2            # null d_x
    assert _raw(kplan, nb, x, 0)[0] == -2                       # all outputs null
    assert _raw(kplan, 0, x, 0)[0] == 0                         # an empty batch
    with pytest.raises(api.NtgError, match="nltc"):             # rows without linear trajectory rows
        kplan.envelope(x, 0, want_rows=True)
    rc, msg = _raw(kplan, nb, x, 0, rlo=buf)
    assert rc == -2 and "nltc" in msg
    viol = torch.zeros(nb, dtype=torch.float64, device="cuda:0")
    rc, msg = _raw(rplan, nb, x, 0, viol=viol)                  # violation outputs without bounds
    assert rc == -2 and "bounds" in msg
    # a row that names outputs of two basis classes: no common pieces for it, the entries are still served
    tspec = cf.config_T()
    tp = api.Plan(tspec, 0)
    tx = dev(np.random.default_rng(2).standard_normal((nb, tspec.nC)))
    with pytest.raises(api.NtgError, match="-4") as e:
        tp.envelope(tx, 0, want_rows=True)
    assert "different basis classes" in str(e.value)
    assert np.isfinite(cpu(tp.envelope(tx, 0))["lo"][:, 6:]).all()
    # host-callback plans
    hp = api.Plan(dataclasses.replace(kincar_spec(), family=-1), 0)
    with pytest.raises(api.NtgError, match="-4"):
        hp.envelope(x, 0)


# ---------------- a loaded module ----------------
def test_unicycle_module_entries_match_the_oracle():
    """no callback is involved: the call reads the plan's spline spaces only, so a loaded family is served like a built-in one"""
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    fam = api.load_family(family.build_module(os.path.join(ROOT, "ntg_amd", "modules", "unicycle.hip")))
    spec, nb, nsub = cf.config_U(fam), 3, 1
    p = api.Plan(spec, 0)
    x = np.random.default_rng(9).standard_normal((nb, spec.nC))
    got = cpu(p.envelope(dev(x), nsub))
    olo, ohi = eo.entry_envelope(spec, x, nsub)
    sl = eo.slack(spec, x)[:, :, None]
    within(got["lo"], olo, sl, "unicycle lo"); within(got["hi"], ohi, sl, "unicycle hi")
