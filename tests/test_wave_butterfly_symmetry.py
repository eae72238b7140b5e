"""The halving butterfly of wave_ops.hpp (wave_sum_many: halve_step over lane bits 1, 2, 4, 8, then xsum_rows over 16 and 32), restated
in numpy over 64 lanes with every addition in the operand order the device code uses.  Every step forms "own + partner's", and the
partner forms the same two numbers the other way round; an IEEE addition is commutative, so the total of a value is the same bit pattern
whichever of the 16 positions it travels in, whatever travels in the other positions and however many positions are valid (KV).  Callers
may therefore group values into butterflies as is cheapest without moving a bit (DESIGN.md 4d records the grouping of the chain
sweep's slots that was tried on this ground)."""
import functools

import numpy as np
import pytest


def halve_step(inp, kv, n, bit):
    """inp: [64][n] -> [64][n // 2]; out[j] = keep + lane_xchg<bit>(send), padding pairs skipped as the template does"""
    lanes = np.arange(64)
    hi = (lanes & bit) != 0
    out = np.zeros((64, n // 2))
    for j in range(n // 2):
        if (2 * j) * bit >= kv:
            continue
        a = inp[:, 2 * j]
        b = inp[:, 2 * j + 1] if (2 * j + 1) * bit < kv else np.zeros(64)
        keep, send = np.where(hi, b, a), np.where(hi, a, b)
        out[:, j] = keep + send[lanes ^ bit]
    return out


def xsum_rows(t, bit):
    """the permlane swaps leave (lower half's, upper half's) in both partners: the lower half adds own + other, the upper other + own"""
    lanes = np.arange(64)
    first, second = np.where((lanes & bit) == 0, t, t[lanes ^ bit]), np.where((lanes & bit) == 0, t[lanes ^ bit], t)
    return first + second


def wave_sum_many(w, kv):
    """w: [64][16], kv valid -> [64]: lane L holds the total of value L & 15"""
    a = halve_step(w, kv, 16, 1)
    b = halve_step(a, kv, 8, 2)
    c = halve_step(b, kv, 4, 4)
    d = halve_step(c, kv, 2, 8)
    return xsum_rows(xsum_rows(d[:, 0], 16), 32)


def _probes():
    rng = np.random.default_rng(11)
    mixed = rng.normal(size=64) * 10.0 ** rng.integers(-12, 13, size=64)   # cancellation: the order of the additions shows in the bits
    with_nan = mixed.copy(); with_nan[37] = np.nan
    zeros = np.full(64, -0.0)                                             # total -0.0: one +0.0 anywhere in its tree would flip the sign
    some_zeros = mixed.copy(); some_zeros[::3] = -0.0
    with_inf = mixed.copy(); with_inf[5] = np.inf
    return {"mixed": mixed, "nan": with_nan, "minus_zero": zeros, "some_minus_zero": some_zeros, "inf": with_inf}


PROBES = _probes()


@functools.lru_cache(maxsize=None)
def _others_base(seed):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(64, 16)) * 10.0 ** rng.integers(-12, 13, size=(64, 16))
    o[rng.random((64, 16)) < 0.05] = np.nan
    o[rng.random((64, 16)) < 0.05] = -0.0
    return o


def _others(seed):
    return _others_base(seed).copy()


def test_restatement_sums():
    """the restatement is a sum: exact on small integers, every lane of a column receives the total"""
    w = np.random.default_rng(5).integers(-1000, 1000, size=(64, 16)).astype(np.float64)
    t = wave_sum_many(w, 16)
    assert np.array_equal(t, w.sum(axis=0)[np.arange(64) & 15])


@pytest.mark.parametrize("probe", list(PROBES))
def test_total_does_not_depend_on_position_or_company(probe):
    v = PROBES[probe]
    seen = set()
    for kv in (4, 10, 14, 16):
        for pos in range(kv):
            for seed in ((1, 2) if pos % 5 == 0 else (1,)):
                w = _others(seed)
                w[:, kv:] = 0.0   # the callers' padding
                w[:, pos] = v
                t = wave_sum_many(w, kv)
                got = t[np.arange(64) & 15 == pos].view(np.int64)
                assert (got == got[0]).all(), (kv, pos)   # all four rows hold the same bits
                seen.add(int(got[0]))
    assert len(seen) == 1, (probe, sorted(seen))
    if probe == "minus_zero":
        assert seen == {int(np.array(-0.0).view(np.int64))}
    if probe == "nan":
        assert np.isnan(np.array(seen.pop(), dtype=np.int64).view(np.float64))
