"""ntg_batch_envelope_sos / ntg_plan_sos_rows without a GPU: the entry points are exported and declared with their argument lists, the
definition's key sentences are in the header, the ctypes binding carries the argument types, Plan.envelope_sos and Plan.sos_rows exist, a
null plan is an argument error -- and the exact oracle the GPU tests compare against (tests/envelope_sos_oracle.py) encloses the rows it
bounds: 33 samples per piece, both ends included, evaluated in double precision through scipy's BSpline.  The oracle's bounds are exact and
rounded once, the samples carry double rounding, so the enclosure is asserted to within sos_slack."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import envelope_oracle as eo
import envelope_sos_oracle as so
from ntg_amd import configs as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSAMP = 33


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_entry_points_are_exported_and_declared(built):
    from ntg_amd import api
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "ntg_amd.h")).read()
    for name, want in (("ntg_plan_sos_rows", "const ntg_plan *p, int *flags"),
                       ("ntg_batch_envelope_sos", "const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper, "
                                                  "double *d_q_lo, double *d_q_hi, double *d_viol, int *d_where, void *stream")):
        assert re.search(r"\bT %s$" % name, syms, re.M), name + " is not exported"
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, name + " is not declared in include/ntg_amd.h"
        assert " ".join(m.group(1).split()) == want
    assert re.search(r"#define NTG_SOS_MAXTERMS 4\b", hdr)
    assert re.search(r"^ \*   ntg_batch_envelope_sos\s+nothing in the reference bounds a row between samples", hdr, re.M)
    assert "constraints.c:119-160" in hdr


def test_the_definition_is_part_of_the_contract(built):
    hdr = " ".join(re.sub(r"^ \*", "", open(os.path.join(ROOT, "include", "ntg_amd.h")).read(), flags=re.M).split())   # comment leaders off, lines joined
    for sentence in ("c_j(z) = sum_{t < nt_j} (z[v_t] - s_t)^2",
                     "s_t = const_t + (pidx_t >= 0 ? prm_row_j[pidx_t] : 0)",
                     "Loaded modules declare nothing",
                     "Then p_i = beta_i - s_t",
                     "its polygon is the single point 0 and p_0 = -s_t",
                     "g_m = sum_{i+j=m} W_d[i][j] p_i p_j, i ascending",
                     "W_d[i][j] = C(d,i) C(d,j) / C(2d,m)",
                     "degree-elevated to D = max_t 2 d_t",
                     "summed in term order",
                     "lo = -inf, hi = +inf on the live pieces, which is no statement",
                     "the largest max(l - lo, hi - u, 0) over certified rows and pieces",
                     "smallest row * npc + piece",
                     "S_t = max_i |c_{o,i}| (2(k-1)/h_min)^r + |s_t|",
                     "2^-40 * sum_t S_t^2",
                     "No scratch allocation and no floating-point atomics",
                     "a partial certificate must not read as a whole one"):
        assert sentence in hdr, sentence


def test_binding_carries_argtypes(built):
    from ntg_amd import api
    L = api.lib()
    assert list(L.ntg_batch_envelope_sos.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    assert list(L.ntg_plan_sos_rows.argtypes) == [C.c_void_p, C.POINTER(C.c_int)]
    assert callable(getattr(api.Plan, "envelope_sos", None)) and callable(getattr(api.Plan, "sos_rows", None))


def test_calls_that_need_no_device(built):
    """a null plan is an argument error wherever the call runs"""
    from ntg_amd import api
    L = api.lib()
    assert L.ntg_batch_envelope_sos(None, 4, None, 0, None, None, None, None, None, None, None) == -2
    assert "null plan" in L.ntg_last_error().decode()
    assert L.ntg_batch_envelope_sos(None, 0, None, 9, None, None, None, None, None, None, None) == -2   # before the empty batch's 0
    assert L.ntg_plan_sos_rows(None, None) == -2


def test_oracle_flags():
    assert so.flags(cf.config_O(ninterv=4)).tolist() == [1]
    assert so.flags(cf.config_OF(3, ninterv=5)).tolist() == [1, 1, 1]
    assert so.flags(cf.config_D(ninterv=8)).tolist() == [1, 1]
    assert so.flags(cf.config_T()).tolist() == [0, 0]          # row 0 names outputs of two basis classes
    assert so.flags(cf.config_E(ninterv=4)).tolist() == [0, 0, 0, 0]


def sampled_rows(spec, x, nsub):
    """the declared rows at NSAMP times of every piece: [nb, nnltc, npc, NSAMP]"""
    nb = x.shape[0]
    npc = max(spec.kninterv) << nsub
    z = np.zeros((nb, npc, NSAMP, spec.nz))
    iz = eo.flag_index(spec)
    for o, sl in enumerate(eo.coef_slices(spec)):
        for r in range(spec.maxderiv[o]):
            z[:, :, :, iz[o] + r] = eo.sample_piece(spec.knots[o], spec.order[o], spec.mult[o], x[:, sl], r, nsub, NSAMP)
    return np.moveaxis(so.rows_numpy(spec, z), -1, 1)


@pytest.mark.parametrize("nsub", [0, 2])
@pytest.mark.parametrize("name", ["O", "D"])
def test_oracle_encloses_samples(name, nsub):
    spec = cf.config_O(ninterv=4) if name == "O" else cf.config_D(ninterv=8)
    x = np.random.default_rng(5 if name == "O" else 6).standard_normal((3, spec.nC))
    if name == "O":
        x[:, :spec.ncoef[0]] += 20.0   # near the obstacle's centre: the shift matters
    lo, hi = so.row_envelope(spec, x, nsub)
    assert lo.shape == (3, spec.nnltc, max(spec.kninterv) << nsub) and np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
    rows = sampled_rows(spec, x, nsub)
    sl = so.sos_slack(spec, x)[:, :, None, None]
    below, above = (lo[..., None] - rows) / sl, (rows - hi[..., None]) / sl
    worst = float(max(below.max(), above.max()))
    print(f"config {name} nsub {nsub}: samples outside the exact bounds by at most {worst:.3g} slack")
    assert worst <= 1.0
    # halving the pieces twice shrinks the enclosure: the bounds are those of the row, not of something wider
    if nsub == 2:
        lo0, hi0 = so.row_envelope(spec, x, 0)
        assert (lo.reshape(3, spec.nnltc, -1, 4).min(axis=3) >= lo0 - sl[..., 0]).all() and (hi.reshape(3, spec.nnltc, -1, 4).max(axis=3) <= hi0 + sl[..., 0]).all()
        tight = (hi - lo).reshape(3, spec.nnltc, -1, 4).max(axis=3)
        assert (tight <= (hi0 - lo0) + sl[..., 0]).all() and (tight < 0.75 * (hi0 - lo0)).any()
