"""An exact statement of ntg_batch_envelope_sos's definition (include/ntg_amd.h) in Python fractions, for the tests -- by another route than
the kernel's.

The kernel extracts Bezier polygons by the blossom, differences them, cuts them by de Casteljau and multiplies polygons.  Here, for every
knot interval, the polynomial of each named entry comes from de Boor's recursion run on polynomials in the local parameter, in exact
rational arithmetic on the double inputs; it is differentiated, restricted to the piece, shifted, squared and summed in the POWER basis;
only the row's polynomial is converted to the Bernstein basis of the piece, at the row's degree D, and lo / hi are rounded to double at
the very end.  Nothing here rounds before that, so the only error a comparison sees is the kernel's.

The row declarations are restated from the families' formulas (ntg_amd/configs.py: config_O, config_OF, config_D; testfam's row 0 is
z_0^2 + z_L^2 with L the last output, its row 1 has a cosine), not read from the library.
"""
from fractions import Fraction as Fr
from math import comb

import numpy as np

from ntg_amd.spec import FAM_OBSTACLE, FAM_OBSTACLE_FIELD, FAM_QUADROTOR, FAM_TESTFAM

QUAD_G = 9.81
MAXTERMS = 4


def declaration(spec):
    """per nonlinear trajectory row: None (not a sum of squares) or its terms [(flag entry v, constant, index into the row's parameters or -1)]"""
    if spec.family == FAM_OBSTACLE:        # (x - 20)^2 + (y - 0.5)^2
        rows = [[(0, 20.0, -1), (3, 0.5, -1)]]
    elif spec.family == FAM_OBSTACLE_FIELD:  # (x - cx_j)^2 + (y - cy_j)^2, parameters [cx_0, cy_0, cx_1, ...]
        rows = [[(0, 0.0, 0), (3, 0.0, 1)] for _ in range(spec.nnltc)]
    elif spec.family == FAM_QUADROTOR:     # thrust^2 = x''^2 + y''^2 + (z'' + g)^2, speed^2 = x'^2 + y'^2 + z'^2; 5 flag entries per output
        rows = [[(2, 0.0, -1), (7, 0.0, -1), (12, -QUAD_G, -1)], [(1, 0.0, -1), (6, 0.0, -1), (11, 0.0, -1)]]
    elif spec.family == FAM_TESTFAM:       # z_0^2 + z_L^2; z_0' z_L'' - cos(z_0)
        rows = [[(0, 0.0, -1), (3 * (spec.nout - 1), 0.0, -1)], None]
    else:
        rows = []
    return (rows + [None] * spec.nnltc)[:spec.nnltc]


NPARAM_ROW = {FAM_OBSTACLE_FIELD: 2}


def entry_of(spec, v):
    """flag entry -> (output, derivative order)"""
    iz = np.concatenate([[0], np.cumsum(spec.maxderiv)])
    o = int(np.searchsorted(iz, v, side="right") - 1)
    return o, int(v - iz[o])


def same_class(spec, a, b):
    return (spec.order[a] == spec.order[b] and spec.mult[a] == spec.mult[b] and spec.kninterv[a] == spec.kninterv[b] and
            spec.maxderiv[a] == spec.maxderiv[b] and np.array_equal(spec.knots[a], spec.knots[b]))


def row_plan(spec):
    """per row: (flag, output whose pieces the row has, terms as (o, r, constant, parameter offset or -1), D)"""
    out = []
    for j, terms in enumerate(declaration(spec)):
        if terms is None:
            out.append((0, 0, [], 0)); continue
        tt = [entry_of(spec, v) + (c, (j * NPARAM_ROW.get(spec.family, 0) + pi) if pi >= 0 else -1) for v, c, pi in terms]
        o0 = tt[0][0]
        if not all(same_class(spec, o, o0) for o, *_ in tt):
            out.append((0, o0, [], 0)); continue
        out.append((1, o0, tt, max(2 * max(spec.order[o] - 1 - r, 0) for o, r, *_ in tt)))
    return out


def flags(spec):
    return np.array([f for f, *_ in row_plan(spec)], dtype=np.int32)


# ---------------- polynomials in the power basis, coefficient lists of Fractions, lowest degree first ----------------
def p_add(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def p_mul(a, b):
    out = [Fr(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def p_diff(a):
    return [i * a[i] for i in range(1, len(a))] or [Fr(0)]


def p_affine(a, s0, w):
    """a(s0 + w u) as a polynomial in u"""
    out, pw = [Fr(0)], [Fr(1)]
    for c in a:
        out = p_add(out, [c * x for x in pw])
        pw = p_mul(pw, [s0, w])
    return out


def aug_knots(brk, k, m):
    brk = [Fr(float(x)) for x in brk]
    return [brk[0]] * k + [x for x in brk[1:-1] for _ in range(k - m)] + [brk[-1]] * k


def interval_poly(t, k, m, c, j, brk):
    """the spline on knot interval j as a polynomial in the local parameter s (time = a + h s), by de Boor's recursion on polynomials"""
    mu = k - 1 + j * (k - m)
    a, h = Fr(float(brk[j])), Fr(float(brk[j + 1])) - Fr(float(brk[j]))
    d = {i: [Fr(float(c[i]))] for i in range(mu - k + 1, mu + 1)}
    for r in range(1, k):
        nd = {}
        for i in range(mu - k + 1 + r, mu + 1):
            den = t[i + k - r] - t[i]
            al = [(a - t[i]) / den, h / den]                 # alpha(s)
            nd[i] = p_add(p_mul([1 - al[0], -al[1]], d[i - 1]), p_mul(al, d[i]))
        d = nd
    return d[mu], h


def to_bernstein(a, D):
    a = list(a) + [Fr(0)] * (D + 1 - len(a))
    assert all(x == 0 for x in a[D + 1:]), "the polynomial's degree exceeds D"
    return [sum(Fr(comb(i, n), comb(D, n)) * a[n] for n in range(i + 1)) for i in range(D + 1)]


def row_envelope(spec, x, nsub, params=None, knots=None):
    """q_lo, q_hi [nb, nnltc, npc] of the definition.  params [nb, nparam]; knots [nb, l + 1]: every problem's own breaks, for every output
    (per-problem grids)"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb, n = x.shape[0], 1 << nsub
    npc = max(spec.kninterv) << nsub
    lo = np.full((nb, spec.nnltc, npc), np.inf); hi = np.full_like(lo, -np.inf)
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])
    for b in range(nb):
        polys = {}   # (output, interval) -> polynomial, h

        def poly(o, j):
            if (o, j) not in polys:
                brk = spec.knots[o] if knots is None else knots[b]
                t = aug_knots(brk, spec.order[o], spec.mult[o])
                polys[(o, j)] = interval_poly(t, spec.order[o], spec.mult[o], x[b, off[o]:off[o + 1]], j, brk)
            return polys[(o, j)]

        for row, (flag, o0, terms, D) in enumerate(row_plan(spec)):
            live = spec.kninterv[o0] << nsub
            if not flag:
                lo[b, row, :live] = -np.inf; hi[b, row, :live] = np.inf
                continue
            for j in range(spec.kninterv[o0]):
                full = []
                for o, r, c, po in terms:
                    p, h = poly(o, j)
                    for _ in range(r):
                        p = [v / h for v in p_diff(p)]
                    s = Fr(float(c)) + (Fr(float(params[b, po])) if po >= 0 else 0)
                    full.append(p_add(p, [-s]))
                for i in range(n):
                    tot = [Fr(0)]
                    for p in full:
                        pp = p_affine(p, Fr(i, n), Fr(1, n))
                        tot = p_add(tot, p_mul(pp, pp))
                    bz = to_bernstein(tot, D)
                    lo[b, row, j * n + i] = float(min(bz)); hi[b, row, j * n + i] = float(max(bz))
    return lo, hi


def sos_slack(spec, x, params=None, knots=None):
    """[nb, nnltc]: 2^-40 sum_t S_t^2, S_t = max_i |c_{o,i}| (2 (k - 1) / h_min)^r + |s_t|; 0 for a row without a statement"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    out = np.zeros((x.shape[0], spec.nnltc))
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])
    for row, (flag, _, terms, _) in enumerate(row_plan(spec)):
        for o, r, c, po in terms:
            hmin = np.diff(np.asarray(spec.knots[o], dtype=np.float64)).min() if knots is None else np.diff(np.asarray(knots), axis=1).min(axis=1)
            s = c + (params[:, po] if po >= 0 else 0.0)
            S = np.abs(x[:, off[o]:off[o + 1]]).max(axis=1) * (2.0 * (spec.order[o] - 1) / hmin) ** r + np.abs(s)
            out[:, row] += 2.0 ** -40 * S * S
    return out


def rows_numpy(spec, z, params=None):
    """the declared rows from flag values z [nb, ..., nz] in double precision: [nb, ..., nnltc] (NaN for a row without a statement)"""
    z = np.asarray(z, dtype=np.float64)
    out = np.full(z.shape[:-1] + (spec.nnltc,), np.nan)
    iz = np.concatenate([[0], np.cumsum(spec.maxderiv)])
    for row, (flag, _, terms, _) in enumerate(row_plan(spec)):
        if not flag:
            continue
        acc = 0.0
        for o, r, c, po in terms:
            s = c + (params[:, po].reshape((-1,) + (1,) * (z.ndim - 2)) if po >= 0 else 0.0)
            acc = acc + (z[..., iz[o] + r] - s) ** 2
        out[..., row] = acc
    return out


def violation(spec, q_lo, q_hi, lower, upper, inf_bound=1e20):
    """viol [nb], where [nb, 2] of the definition from given bounds of the rows: the largest max(l - lo, hi - u, 0) over certified rows and
    live pieces, the first of equal maxima in the order row * npc + piece"""
    nb, nrow, npc = q_lo.shape
    s0 = spec.nlic + spec.nltc + spec.nlfc + spec.nnlic
    fl = flags(spec)
    viol = np.zeros(nb); where = np.full((nb, 2), -1, dtype=np.int64)
    for b in range(nb):
        v = np.zeros((nrow, npc))
        for i in range(nrow):
            if not fl[i]:
                continue
            l, u = lower[b, s0 + i], upper[b, s0 + i]
            live = ~(np.isposinf(q_lo[b, i]) & np.isneginf(q_hi[b, i]))
            if abs(l) < inf_bound:
                v[i] = np.maximum(v[i], np.where(live, l - q_lo[b, i], 0.0))
            if abs(u) < inf_bound:
                v[i] = np.maximum(v[i], np.where(live, q_hi[b, i] - u, 0.0))
        if v.max() > 0:
            viol[b] = v.max()
            where[b] = divmod(int(np.argmax(v)), npc)
    return viol, where
