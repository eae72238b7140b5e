"""The CPU restatement of ntg_batch_verify (tests/verify_oracle.py) alone, no GPU and no library call: it reports every clean case of
tests/test_gpu_verify.py as clean, the three planted defects of tests/modules/miswired_family.hpp exactly where they were planted, and
nothing else.  Its figures define the tolerances of the GPU tests (100 N, N = the largest err and leak over the clean slots), so the
conditions on the inputs are asserted here: N <= 1e-8 for coefficients 0.3 * normal, every planted defect >= 1e-3."""
import numpy as np
import pytest

from ntg_amd import configs as cf
import verify_oracle as vo
from gpu_common import SPECS

NMAX, PLANTED_MIN, AMP = 1e-8, 1e-3, 0.3
BUILTIN = {"A": SPECS["A"], "K0": SPECS["K0"], "T": SPECS["T"], "O4": lambda: cf.config_O(ninterv=4), "D8": SPECS["D8"], "E8": SPECS["E8"],
           "M": SPECS["M"], "E8x3": lambda: cf.config_E(ninterv=8, narms=3)}


def coefficients(spec, nb, seed=21):
    return AMP * np.random.default_rng(seed).normal(size=(nb, spec.nC))


@pytest.mark.parametrize("name", list(BUILTIN))
def test_builtin_families_are_clean(name):
    spec, cbs, _, _ = vo.builtin_case(BUILTIN[name]())
    ref = vo.restate(spec, coefficients(spec, 2), cbs)
    N = vo.floor(ref)
    print(f"{name}: N {N:.3e}  err {ref['err'].max(axis=0)}  leak {ref['leak'].max(axis=0)}")
    assert N <= NMAX
    used = np.array([n > 0 for n, _, _ in vo.slot_setup(spec)])
    assert (ref["err"][:, ~used] == 0).all() and (ref["where"][:, ~used] == -1).all() and (ref["leak"][:, ~used] == 0).all()


def test_modules_and_parameters_are_clean():
    for label, (spec, cbs, setp, _) in (("OF", vo.obstacle_field_case(2)), ("TR", vo.tracking_case(64, 2)), ("U", vo.unicycle_case(64))):
        ref = vo.restate(spec, coefficients(spec, 2), cbs, set_problem=setp)
        N = vo.floor(ref)
        print(f"{label}: N {N:.3e}  err {ref['err'].max(axis=0)}  leak {ref['leak'].max(axis=0)}")
        assert N <= NMAX


def test_planted_defects_are_found_where_they_were_planted():
    spec, cbs, _, _ = vo.miswired_case(64)
    nb = 3
    ref = vo.restate(spec, coefficients(spec, nb), cbs)
    N = vo.floor(ref, vo.PLANTED)
    print(f"miswired: N {N:.3e}\nerr {ref['err']}\nleak {ref['leak']}\nwhere {ref['where'].tolist()}\nleak_where {ref['leak_where'].tolist()}")
    assert N <= NMAX
    P = spec.nbps
    for s, (kind, fn, entry) in vo.PLANTED.items():
        val, wh = (ref["err"], ref["where"]) if kind == "err" else (ref["leak"], ref["leak_where"])
        assert (val[:, s] >= PLANTED_MIN).all(), (s, val[:, s])
        assert (wh[:, s, 0] == fn).all() and (wh[:, s, 2] == entry).all(), (s, wh[:, s])
        assert (wh[:, s, 1] == (P - 1 if s == 2 else wh[:, s, 1])).all() and (wh[:, s, 1] >= 0).all() and (wh[:, s, 1] < P).all()
        other = ref["leak"] if kind == "err" else ref["err"]
        assert (other[:, s] <= N).all()   # the planted slot's other figure is clean
    # ... and nothing else: within the planted slots every OTHER (function, entry) of the dense tables is at the floor
    for b in range(nb):
        for s, (kind, fn, entry) in vo.PLANTED.items():
            tab = (ref["e"] if kind == "err" else ref["l"])[b][s].copy()
            tab[fn, :, entry] = 0.0
            named = vo.slot_setup(spec)[s][2]
            sel = named if kind == "err" else ~named
            assert tab[:, :, sel].max() <= NMAX


def test_maximum_rule():
    """ties go to the smallest (function * nbps + breakpoint) * nz + entry, a zero maximum has no place, a NaN beats every number"""
    tab = np.zeros((2, 3, 4)); sel = np.array([True, True, False, True])
    assert vo._maximum(tab, sel) == (0.0, [-1, -1, -1])
    tab[1, 0, 1] = 0.5; tab[0, 2, 3] = 0.5; tab[0, 1, 2] = 9.0   # (entry 2 is not selected)
    assert vo._maximum(tab, sel) == (0.5, [0, 2, 3])
    tab[1, 2, 0] = np.nan
    v, w = vo._maximum(tab, sel)
    assert np.isnan(v) and w == [1, 2, 0]
    assert vo._maximum(tab, ~sel) == (9.0, [0, 1, 2])
