"""The time certificates -- Plan.envelope, Plan.envelope_sos, Plan.extrema -- reproduce recorded results bit for bit.  The fixture
tests/golden/cert_calls.npz was recorded on the GPU with tools/record_cert_golden.py from the library of the commit before the three calls
got one row-polygon builder and one host setup; the cases are in tests/cert_golden_cases.py.  Integers are compared exactly, doubles by
their bit patterns with NaNs by position, refusals by their text.  The first test needs no GPU: it holds the fixture to what the cases claim
to reach."""
import os

import numpy as np
import pytest

import cert_golden_cases as wc
import extrema_oracle as xo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cert_calls.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_fixture_holds_what_the_cases_claim(golden):
    assert {k.split("/")[0] for k in golden.files} == set(wc.CASES)
    assert golden["FULL80/ext_s1/status"][0, 0] == xo.FULL and golden["FULL80/ext_s1/npieces"][0, 0] == 80   # two passes over the intervals
    for name in xo.CASES:
        assert (golden[name + "/ext_d0/status"] == xo.DEPTH).any(), name
        assert np.isin(golden[name + "/ext/status"], (xo.OK, xo.NONE)).all(), name
    assert (golden["T3/ext/status"][:, 2] == xo.NONE).all() and "T3/ext_b/viol" not in golden.files      # a row with flag 0
    assert (golden["T3/sos0/q_lo"][:, 1] == -np.inf).all() and "is not certified" in str(golden["T3/sos0_b/error"])
    for name, calls in (("O4", "ext sos0 sos2"), ("OF5", "ext sos0 sos2"), ("D8", "ext sos0 sos2"), ("G4", "ext sos0 sos2"), ("K3", "ext env0 env2"), ("T3", "env0 env2")):
        for call in calls.split():
            assert (golden["%s/%s_b/viol" % (name, call)] > 0).any() and (golden["%s/%s_b/where" % (name, call)] >= 0).any(), (name, call)
    st = golden["K3_nan/ext/status"]   # the NaN is in the second of three problems; row 0 does not name it
    assert (st[1, 1:] == xo.NAN).all() and (st[(0, 2), :] == xo.OK).all() and st[1, 0] == xo.OK
    assert np.isnan(golden["K3_nan/ext/ext"][1, 1:]).all() and np.isnan(golden["K3_nan/env0_b/viol"]).tolist() == [False, True, False]
    assert np.isnan(golden["K3_nan/env2/row_lo"][1, 1:, :4]).all() and not np.isnan(golden["K3_nan/env2/row_lo"][1, 0]).any()
    assert "T/env1/lo" in golden.files and "no nonlinear trajectory row" in str(golden["T/sos1/error"])   # outputs in different basis classes
    assert golden["K3_zero/env0/row_lo"].shape[1] == 4 and (golden["K3_zero/ext/ext"][:, 3] == 0.0).all()   # the plan with the row of zeros is taken
    assert golden["D8/sos0/q_lo"].shape[1] == 2 and golden["G4/env2/lo"].shape[0] == 5 and golden["O4/ext/ext"].shape[0] == xo.NBIG


@pytest.mark.gpu
@pytest.mark.parametrize("name", wc.CASES)
def test_certificates_bitwise(golden, name):
    got = wc.run_case(name)
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
