"""Plan.interp reproduces recorded flags bit for bit, in one chunk and in several.  The fixture tests/golden/interp_calls.npz was recorded
on the GPU with tools/record_cert_golden.py (set `interp`) from the library of the commit before ntg_batch_interp_strided got its time
tables from the builder ntg_batch_check, ntg_batch_cost and ntg_batch_verify use (plan_times.cpp); the cases are in
tests/interp_golden_cases.py.  Doubles are compared by their bit patterns.  The first test needs no GPU: it holds the fixture to what the
cases claim to contain."""
import ctypes as C
import os

import numpy as np
import pytest

import interp_golden_cases as ic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interp_calls.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def stored(golden, name):
    return {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "/")}


def same_bits(g, w):
    return g.dtype == w.dtype and g.shape == w.shape and not np.isnan(w).any() and np.array_equal(g.view(np.int64), w.view(np.int64))


def test_the_fixture_holds_what_the_cases_claim(golden):
    from ntg_amd import configs as cf
    assert {k.split("/")[0] for k in golden.files} == set(ic.CASES) and os.path.getsize(GOLDEN) < 100 * 1024
    for name in ic.CASES:
        inp, st = ic.inputs(name), stored(golden, name)
        assert set(st) == set(inp) | {"z"}, name
        assert all(same_bits(st[k], v) for k, v in inp.items()), name   # the cases still generate the inputs that were recorded
    # T: two basis classes; both ends, and a knot of either class between its two neighbouring doubles
    spec = cf.config_T()
    t = golden["T/times"]
    assert len({(k, l) for k, l in zip(spec.order, spec.kninterv)}) == 2 and golden["T/z"].shape == (ic.NB, 9, spec.nz)
    assert t[0] == spec.bps[0] and t[1] == spec.bps[-1]
    for kn in (spec.knots[0][2], spec.knots[-1][3]):
        i = int(np.flatnonzero(t == kn)[0])
        assert 0 < kn < 2 and t[i - 1] == np.nextafter(kn, -np.inf) and t[i + 1] == np.nextafter(kn, np.inf)
    # PP: every problem at both of its own ends and around its own knot 2; PP0: the same around knot 2 of problem 1, for everyone
    kn, t = golden["PP/knots"], golden["PP/times"]
    assert t.shape == (ic.NB, 7) and golden["PP/z"].shape == (ic.NB, 7, cf.config_M().nz) and np.ptp(kn[:, -1]) > 0.1
    assert (t[:, 0] == kn[:, 0]).all() and (t[:, 1] == kn[:, -1]).all() and (t[:, 3] == kn[:, 2]).all()
    assert (t[:, 2] == np.nextafter(kn[:, 2], -np.inf)).all() and (t[:, 4] == np.nextafter(kn[:, 2], np.inf)).all()
    t = golden["PP0/times"]
    assert t.shape == (7,) and t[0] == kn[:, 0].max() and t[1] == kn[:, -1].min() and t[3] == kn[1, 2]
    assert t[2] == np.nextafter(kn[1, 2], -np.inf) and t[4] == np.nextafter(kn[1, 2], np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ic.CASES)
def test_interp_bitwise(golden, name):
    st = stored(golden, name)
    assert same_bits(ic.run(name, st), st["z"])


def _debug_interp(plan, x, times, stride, cap):
    """ntg_debug_batch_interp_strided: ntg_batch_interp_strided with the scratch cap of the per-problem time tables stated; -> (rc, z)"""
    import torch
    from ntg_amd import api
    L = api.lib()
    L.ntg_debug_batch_interp_strided.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong]
    nb, nt = x.shape[0], times.shape[-1]
    z = torch.full((nb, nt, plan.spec.nz), float("nan"), dtype=torch.float64, device=x.device)
    rc = L.ntg_debug_batch_interp_strided(plan.h, nb, x.data_ptr(), nt, times.data_ptr(), stride, z.data_ptr(), None, cap)
    torch.cuda.synchronize()
    return rc, z


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["PP", "PP0"])
def test_interp_in_chunks(golden, name):
    """the batch of 5 in chunks of 1, of 2 (2 + 2 + 1: an uneven tail) and in one piece: each the uncapped call and the recorded flags bit
    for bit; a cap that is not positive is refused with the words of check, cost and verify"""
    import torch
    from gpu_common import dev
    from ntg_amd import api
    st = stored(golden, name)
    plan = ic.plan_of(name, st)
    xd, td = dev(st["x"]), dev(st["times"])
    stride = 0 if name == "PP0" else td.shape[1]
    whole = plan.interp(xd, td)
    assert same_bits(whole.cpu().numpy(), st["z"])
    spec, nt = plan.spec, td.shape[-1]
    per = nt * (spec.order[0] * spec.maxderiv[0] * 8 + 4)   # bytes of one problem's tables: its basis blocks and offsets at the times
    for cap, chunk in ((1, 1), (per, 1), (2 * per + 8, 2), (3 * per - 1, 2), (ic.NB * per, ic.NB), (64 << 20, ic.NB)):
        rc, z = _debug_interp(plan, xd, td, stride, cap)
        assert rc == 0, api.lib().ntg_last_error().decode()
        assert torch.equal(z, whole), (cap, chunk)
    for cap in (0, -1):
        rc, z = _debug_interp(plan, xd, td, stride, cap)
        assert rc != 0 and "scratch cap must be positive" in api.lib().ntg_last_error().decode() and torch.isnan(z).all()
