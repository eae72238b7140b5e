"""Shared grids with uneven knots and an uneven number of breakpoints per knot interval (a helper module, not a conftest).

Every other plan of the suite has uniform knots and the same number of breakpoints in every knot interval (ntg_amd/configs.py builds every
grid with linspace_c).  The grids here are deterministic, so anyone can rebuild them:

    knots   kn_j = T (u_j + a u_j (1 - u_j)),  u_j = j / l            (a = 0.4: the first interval is 1.9 times as long as the last)
    bps     counts[j] breakpoints in knot interval j, the first of them ON the knot, equally spaced inside the interval; then T

so the last group holds counts[-1] + 1 breakpoints (it takes the end point).  ulp=True moves the last breakpoint of the third interval
to one ulp below the fourth knot: the largest double that still belongs to the third interval.
"""
import dataclasses

import numpy as np

from ntg_amd import configs as cf

C20 = (5, 3, 6, 4, 3, 6, 3, 4, 5, 4, 3, 6, 5, 6, 3, 5, 4, 5, 6, 4)          # P = 91: 20 groups of 3 .. 6 breakpoints
C16 = (5, 3, 4, 6, 4, 5, 4, 3, 4, 5, 4, 6, 4, 5, 6, 5)                      # P = 74: the 16-interval instances
C20_7 = C20[:7] + (7,) + C20[8:]                                            # P = 94: one group of 7 (more than a group table holds)
C20_0 = C20[:9] + (0,) + C20[10:]                                           # P = 87: a knot interval without a breakpoint
C20_thin = (5, 3, 6, 4, 2, 1, 1, 1, 2, 4, 3, 6, 5, 6, 3, 5, 4, 5, 6, 4)     # P = 77: too few breakpoints in the middle, singular reduced Hessian
C8 = (5, 3, 6, 4, 3, 6, 4, 4)                                               # P = 36: config_D(ninterv=8), config_E(ninterv=8, narms=2)
COUNTS = {"C20": C20, "C16": C16, "C20_7": C20_7, "C20_0": C20_0, "C20_thin": C20_thin, "C8": C8}
ULP = {"C20": True}                                                         # the list that carries the one-ulp breakpoint


def grid(counts, T, a=0.4, ulp=False):
    """(knots [l + 1], bps [sum(counts) + 1]) of the docstring above"""
    l = len(counts)
    u = np.arange(l + 1) / l
    kn = T * (u + a * u * (1 - u))
    kn[0] = 0.0; kn[-1] = T
    bps = [kn[j] + (i / c) * (kn[j + 1] - kn[j]) for j, c in enumerate(counts) for i in range(c)] + [T]
    if ulp:
        bps[sum(counts[:3]) - 1] = np.nextafter(kn[3], -np.inf)
    bps = np.array(bps, dtype=np.float64)
    assert np.all(np.diff(kn) > 0) and np.all(np.diff(bps) > 0)
    return kn, bps


def on(spec, counts, **kw):
    """spec on the uneven grid of `counts` over its own horizon (every output on the same knots)"""
    assert all(l == len(counts) for l in spec.kninterv)
    kn, bps = grid(counts, float(spec.knots[0][-1]), **kw)
    return dataclasses.replace(spec, bps=bps, knots=[kn.copy() for _ in range(spec.nout)], name=f"{spec.name}@uneven{len(bps)}")


def kincar(ncars, name):
    """_kincar_spec(ncars, 6, 3, l, 2, 5.0, ...) on the count list `name`"""
    counts = COUNTS[name]
    return on(cf._kincar_spec(ncars, 6, 3, len(counts), 2, 5.0, f"kincar-{2 * ncars}out-{name}"), counts, ulp=ULP.get(name, False))


def O20():
    return on(cf.config_O(ninterv=20), C20, ulp=True)


def O16():
    return on(cf.config_O(ninterv=16), C16)


def D8():
    return on(cf.config_D(ninterv=8), C8)


def E8():
    return on(cf.config_E(ninterv=8, narms=2), C8)


# The solved batches, shared by tests/test_uneven_grids_oracle.py (which asserts on the CPU what the GPU tests rely on) and
# tests/test_gpu_uneven_grids.py: x0 = 1 everywhere.
NB_CONV, NB_FIXED, NB_DEGEN = 8, 16, 4      # kincar problems: to convergence, 50 fixed majors, the degenerate lists C20_0 / C20_thin
SECOND_ORDER = ("O-C20", "O-C16", "D8-C8", "E8-C8")   # the Newton (hessian = 2) and QP (hessian = 3) cases, names of ALL below


def second_order_bounds(name, hessian):
    """bounds of a second-order case's batch.  D8 in the QP mode takes the first 6 problems of quadrotor_bounds(8): the oracle ends
    problem 6 at inform 4 after 1272 majors in that mode."""
    if name in ("O-C20", "O-C16"):
        return cf.obstacle_bounds(12)
    if name == "D8-C8":
        lo, up = cf.quadrotor_bounds(8)
        return (lo, up) if hessian == 2 else (lo[:6].copy(), up[:6].copy())
    assert name == "E8-C8"
    return cf.manipulator_bounds(8, narms=2)


KINCAR_LISTS = ("C20", "C16", "C20_7", "C20_0", "C20_thin")
# the four cases with a reference-code fixture (tests/golden/ref_U*.npz, tests/golden/make_golden.py)
FIXTURES = {"U20": lambda: kincar(3, "C20"), "U16": lambda: kincar(2, "C16"), "UO": O20, "UD8": D8}
# every spec of this module, by a short name
ALL = {f"K{n}-{c}": (lambda n=n, c=c: kincar(n, c)) for c in KINCAR_LISTS for n in (1, 2, 3)}
ALL.update({"O-C20": O20, "O-C16": O16, "D8-C8": D8, "E8-C8": E8})
