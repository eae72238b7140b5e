"""The bisection calls beside Plan.extrema -- Plan.separation, Plan.forms, Plan.ratios -- reproduce recorded results bit for bit.  The fixture
tests/golden/bisect_calls.npz was recorded on the GPU with tools/record_cert_golden.py (set `bisect`) from the library of the commit before
the four calls got one level loop, one LDS layout and one epilogue; the cases are in tests/bisect_golden_cases.py.  Integers are compared
exactly, doubles by their bit patterns with NaNs by position, refusals by their text.  The first test needs no GPU: it holds the fixture to
what the cases claim to reach."""
import os

import numpy as np
import pytest

import bisect_golden_cases as bc
import forms_oracle as fo
import ratios_oracle as ro
import separation_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bisect_calls.npz")
CERT_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "cert_calls.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_fixture_holds_what_the_cases_claim(golden):
    assert {k.split("/")[0] for k in golden.files} == set(bc.CASES)
    assert not [k for k in golden.files if k.endswith("/error")]
    assert os.path.getsize(GOLDEN) < os.path.getsize(CERT_GOLDEN)
    # separation: every pair OK at the working tolerance and past level 0; DEPTH at max_depth = 0; the bad pairs between good ones
    for name in bc.SEP_CASES:
        l = po.inputs(name[:-3], int(name[-1])).spec.kninterv[0]
        assert (golden[name + "/sep/status"] == po.OK).all() and (golden[name + "/sep_thr/status"] == po.OK).all(), name
        assert (golden[name + "/sep/npieces"] > l).any() and (golden[name + "/sep_d0/status"] == po.DEPTH).any(), name
        assert (golden[name + "/sep_d0/npieces"] == l).all(), name
        assert golden[name + "/sep_bad/status"].tolist()[1::2] == [po.BADPAIR] * 3 and (golden[name + "/sep_bad/status"][::2] == po.OK).all(), name
        assert np.isnan(golden[name + "/sep_bad/viol"][1::2]).all() and "sep/viol" not in {k[len(name) + 1:] for k in golden.files if k.startswith(name + "/")}
    for name, l in (("S4-d0", 4), ("S20-d0", 20)):   # with the required distance a pair that keeps it ends at level 0, and goes deeper without it
        at0 = golden[name + "/sep_thr/npieces"] == l   # (the quadrotors of Q8 all come closer than their required distance: none stops there)
        assert at0.any() and (golden[name + "/sep/npieces"][at0] > l).any(), name
    assert (golden["Q8-d0/sep_thr/npieces"] > 8).all() and (golden["Q8-d1/sep_thr/npieces"] > 8).all()
    # forms: the status every case expects; past level 0 but where the list overflows there (L80: all 80 intervals open at level 0, FULL)
    for name in bc.FORM_CASES:
        c = fo.inputs(name)
        l = max(c.spec.kninterv)
        assert (golden[name + "/forms/status"] == c.expect).all(), name
        if c.expect == fo.OK:
            assert (golden[name + "/forms/npieces"] > l).any() and (golden[name + "/forms_s1/npieces"] > l).any(), name
            assert (golden[name + "/forms_b/viol"] > 0).any() and (golden[name + "/forms_b/where"] >= 0).any(), name
        assert (golden[name + "/forms_d0/status"] != fo.OK).any() and golden[name + "/forms_d0/status"].max() <= max(fo.DEPTH, fo.FULL), name
        assert (golden[name + "/forms_s1/npieces"] <= golden[name + "/forms/npieces"]).all(), name
    assert (golden["L80/forms/status"] == fo.FULL).all() and (golden["L80/forms/npieces"] == 80).all()   # two rounds over the intervals
    assert (golden["K4/forms_d0/status"] == fo.DEPTH).any()
    assert max(fo.inputs("D8").spec.order) > 6 and fo.inputs("PP").knots is not None and len(set(fo.inputs("T4").spec.kninterv)) + len(set(fo.inputs("T4").spec.order)) > 2
    # ratios: OK at both tolerances and past level 0; DEPTH, POLE and NAN on RK4; FULL on RK100
    reached = set()
    for name in bc.RATIO_CASES:
        c = ro.inputs(name)
        l = c.spec.kninterv[0]
        for r, ratio in enumerate(c.ratios):
            reached.add(bc.ratio_instance(c.spec, c.forms, [ratio]))
            for call in ("r%d" % r, "r%d_fine" % r):
                assert (golden["%s/%s/status" % (name, call)] == ro.OK).all() and (golden["%s/%s/npieces" % (name, call)] > l).any(), (name, call)
                assert (golden["%s/%s/viol" % (name, call)][:, 0] > 0).any(), (name, call)
    assert reached == {(6, 13), (6, 25), (bc.MAX_ORDER, 25)}
    k4 = ro.inputs("RK4")
    assert bc.ratio_instance(k4.spec, k4.forms, [ro.SLOPE]) == (6, 13) and bc.ratio_instance(k4.spec, k4.forms, [ro.KAPPA2]) == (6, 25)   # degrees 4 and 24
    r8 = ro.inputs("R8")
    assert bc.ratio_instance(r8.spec, r8.forms, r8.ratios) == (bc.MAX_ORDER, 25) and bc.ratio_instance(k4.spec, k4.forms, bc.NAN_RATIOS) == (6, 25)
    for r, ratio in enumerate(k4.ratios):
        assert (golden["RK4/r%d_d3/status" % r] == ro.DEPTH).any()
        assert (golden["RK4/r%d_park/status" % r][7, 0] == ro.POLE) == bool(ratio[1])
        assert (np.delete(golden["RK4/r%d_park/status" % r], 7, axis=0) == ro.OK).all()
    assert golden["RK4/r0_park/npieces"][7, 0] == 4 and golden["RK4/r0_park/viol"][7].tolist() == [0.0, np.inf]
    st = golden["RK4/nan/status"]
    assert (st[5, :2] == ro.NAN).all() and (st[5, 2:] == ro.OK).all() and (np.delete(st, 5, axis=0) == ro.OK).all() and np.isnan(golden["RK4/nan/ext"][5, :2]).all()
    assert (golden["RK100/r0/status"] == ro.OK).all() and (golden["RK100/r0/npieces"] > 100).all()
    assert (golden["RK100/r0_fine/status"] == ro.FULL).all() and (golden["RK100/r0_fine/npieces"] == 100).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", bc.CASES)
def test_bisection_calls_bitwise(golden, name):
    got = bc.run_case(name)
    want = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "/")}
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if w.dtype == np.float64:   # bit patterns (array_equal on the floats would also accept -0.0 == 0.0); a NaN at the same places
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), k
            assert np.array_equal(g.view(np.int64)[~nan], w.view(np.int64)[~nan]), k
        else:
            assert np.array_equal(g, w), k
