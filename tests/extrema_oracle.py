"""ntg_batch_extrema's definition (include/ntg_amd.h) for the tests, and the inputs the CPU and GPU tests share.

  level_oracle   the level algorithm of the definition in float64 (bisect_oracle.levels), on level-0 polygons handed in: from row_polygons
                 (numpy: the interval polygons of envelope_oracle, differenced, multiplied by the Bezier product, elevated, summed) or from
                 exact_polygons rounded.
  exact_extrema  the true minimum and maximum of a row in fractions.Fraction: rational bisection of the exact level-0 Bernstein polygons
                 (the polynomials of envelope_sos_oracle's de Boor recursion, converted once), until the enclosure is narrower than eps.
  slack          2 * envelope_sos_oracle.sos_slack for a quadratic row (2^-39 sum_t S_t^2), 2 * envelope_oracle.row_slack for a linear one.

Rows are numbered as ntg_batch_check numbers them: the nltc linear trajectory rows, then the nnltc nonlinear ones.
"""
import dataclasses
from fractions import Fraction as Fr
from math import comb

import numpy as np

import bisect_oracle as bo
import envelope_oracle as eo
import envelope_sos_oracle as so
from bisect_oracle import CAP, DEPTH, FULL, MAX_DEPTH, NAN, NONE, OK   # (the tests take them from here)
from cert_common import field_x, greville, obstacle_x, rows_spec, scaled_grids   # (the tests and tools take them from here too)
from ntg_amd import configs as cf



# ---------------- rows ----------------
def row_table(spec):
    """per row: (flag, output whose knot intervals the row has, 'lin' | 'sos', terms, D).  Terms of a linear row: (o, r, weight), v ascending,
    r < order only; of a quadratic row: envelope_sos_oracle's (o, r, constant, parameter offset or -1)"""
    out = []
    iz = eo.flag_index(spec)
    ltc = np.asarray(spec.ltc, dtype=np.float64).reshape(spec.nltc, spec.nz)
    for i in range(spec.nltc):
        named = [(o, r, float(ltc[i, iz[o] + r])) for o in range(spec.nout) for r in range(spec.maxderiv[o]) if ltc[i, iz[o] + r] != 0.0]
        o0 = named[0][0] if named else 0
        flag = int(all(so.same_class(spec, o, o0) for o, _, _ in named))
        terms = [(o, r, w) for o, r, w in named if r < spec.order[o]]
        out.append((flag, terms[0][0] if terms else 0, "lin", terms, max([spec.order[o] - 1 - r for o, r, _ in terms] + [0])))
    for flag, o0, terms, D in so.row_plan(spec):
        out.append((flag, o0, "sos", terms, D))
    return out


def flags(spec):
    return np.array([f for f, *_ in row_table(spec)], dtype=np.int32)


def slack(spec, x, params=None, knots=None):
    """[nb, nrow]; knots [nb, l + 1] on per-problem grids"""
    x = np.atleast_2d(x)
    if knots is None:
        lin = 2.0 * eo.row_slack(spec, x)
    else:
        lin = np.stack([2.0 * eo.row_slack(spec, x[b:b + 1], knots[b])[0] for b in range(x.shape[0])]).reshape(x.shape[0], spec.nltc)
    return np.concatenate([lin.reshape(x.shape[0], spec.nltc), 2.0 * so.sos_slack(spec, x, params, knots)], axis=1)


def square(P):
    """Bezier product of the polygons P [..., d + 1] with themselves: [..., 2 d + 1]"""
    d = P.shape[-1] - 1
    G = np.zeros(P.shape[:-1] + (2 * d + 1,))
    for i in range(d + 1):
        for j in range(d + 1):
            G[..., i + j] += comb(d, i) * comb(d, j) / comb(2 * d, i + j) * P[..., i] * P[..., j]
    return G


def row_polygons(spec, x, params=None, knots=None):
    """level-0 polygons in float64: per row None (flag 0) or [nb, l, D + 1].  knots [nb, l + 1]: every problem's own breaks"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb = x.shape[0]
    sls = eo.coef_slices(spec)
    cache = {}

    def polys(o):
        if o not in cache:
            if knots is None:
                cache[o] = eo.piece_polygons(spec.knots[o], spec.order[o], spec.mult[o], x[:, sls[o]], spec.maxderiv[o], 0)
            else:
                per = [eo.piece_polygons(knots[b], spec.order[o], spec.mult[o], x[b:b + 1, sls[o]], spec.maxderiv[o], 0) for b in range(nb)]
                cache[o] = [np.concatenate([p[r] for p in per], axis=0) for r in range(len(per[0]))]
        return cache[o]

    out = []
    for flag, o0, kind, terms, D in row_table(spec):
        if not flag:
            out.append(None); continue
        S = np.zeros((nb, spec.kninterv[o0], D + 1))
        for term in terms:
            o, r = term[0], term[1]
            P = polys(o)[r] if r < spec.order[o] else np.zeros((nb, spec.kninterv[o], 1))
            if kind == "sos":
                c, po = term[2], term[3]
                s = c + (params[:, po] if po >= 0 else 0.0)
                P = square(P - np.broadcast_to(s, (nb,))[:, None, None])
            while P.shape[-1] - 1 < D:
                P = eo.elevate(P)
            S = S + (term[2] * P if kind == "lin" else P)
        out.append(S)
    return out


def exact_polygons(spec, xb, pb=None, kb=None):
    """level-0 polygons of ONE problem in Fractions: per row None or a list over the intervals of D + 1 Fractions"""
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])
    cache = {}

    def poly(o, j):
        if (o, j) not in cache:
            brk = spec.knots[o] if kb is None else kb
            t = so.aug_knots(brk, spec.order[o], spec.mult[o])
            cache[(o, j)] = so.interval_poly(t, spec.order[o], spec.mult[o], xb[off[o]:off[o + 1]], j, brk)
        return cache[(o, j)]

    out = []
    for flag, o0, kind, terms, D in row_table(spec):
        if not flag:
            out.append(None); continue
        rows = []
        for j in range(spec.kninterv[o0]):
            tot = [Fr(0)]
            for term in terms:
                p, h = poly(term[0], j)
                for _ in range(term[1]):
                    p = [v / h for v in so.p_diff(p)]
                if kind == "sos":
                    s = Fr(float(term[2])) + (Fr(float(pb[term[3]])) if term[3] >= 0 else 0)
                    q = so.p_add(p, [-s])
                    tot = so.p_add(tot, so.p_mul(q, q))
                else:
                    tot = so.p_add(tot, [Fr(float(term[2])) * v for v in p])
            rows.append(so.to_bernstein(tot, D))
        out.append(rows)
    return out


# ---------------- the definition ----------------
def level_oracle(polys, kn, tol, max_depth=MAX_DEPTH, sides=3, cap=CAP):
    """one row of one problem: polys [l][D + 1] floats, kn [l + 1] its breaks.  bisect_oracle.levels on single polygons: a dict with ext
    (min_lo, min_hi, max_lo, max_hi), when (t_min, t_max), status, npieces, and for the tests depth, max_open and margin"""
    return bo.levels(bo.POLYGON, [[float(v) for v in B] for B in polys], kn, tol, max_depth, sides, cap)


def _exact_min(polys, eps):
    """(lo, hi), Fractions with lo <= min over the horizon <= hi and hi - lo < eps; hi is attained"""
    pieces = [list(B) for B in polys]
    U = min(min(B[0], B[-1]) for B in pieces)
    while True:
        pieces = [B for B in pieces if min(B) < U]   # the others hold nothing below an attained value
        lo = min([U] + [min(B) for B in pieces])
        if U - lo < eps:
            return lo, U
        nxt = []
        for B in pieces:
            R, L = list(B), [B[0]]
            for r in range(1, len(B)):
                for s in range(len(B) - r):
                    R[s] = (R[s] + R[s + 1]) / 2
                L.append(R[0])
            U = min(U, R[0])
            nxt += [L, R]
        pieces = nxt


def exact_extrema(polys, eps):
    """(min_lo, min_hi, max_lo, max_hi) of one row from its exact level-0 polygons, each enclosure narrower than eps"""
    eps = Fr(float(eps))
    lo, hi = _exact_min(polys, eps)
    nlo, nhi = _exact_min([[-v for v in B] for B in polys], eps)
    return lo, hi, -nhi, -nlo


# ---------------- the inputs of the GPU tests ----------------
def testfam_spec():
    """testfam with its three outputs in one basis class: the linear row and nonlinear row 0 are certified, row 1 (a cosine) is not"""
    t0 = cf.config_T()
    return dataclasses.replace(t0, order=[t0.order[0]] * 3, kninterv=[t0.kninterv[0]] * 3, knots=[np.array(t0.knots[0]) for _ in range(3)])


@dataclasses.dataclass
class Inputs:
    """a plan's spec, nb problems on it, the number of them the exact oracle runs on, and the one tolerance of the case"""
    name: str
    spec: object
    x: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prm: object = None
    knots: object = None    # [nb, l + 1]: per-problem grids
    bps: object = None
    nexact: int = 2
    tol: float = 0.0
    sl: np.ndarray = None   # slack [nb, nrow]
    polys: list = None      # row_polygons

    def kn(self, b, o0=0):
        return self.spec.knots[o0] if self.knots is None else self.knots[b]


NBIG = 67   # leaves the persistent loop a partial last pass
CASES = ["O4", "O20", "OF5", "D8", "T3", "K3", "G4"]
_inputs = {}


def inputs(name):
    """O4 / O20: the obstacle plan on 4 / 20 intervals; OF5: the obstacle field; D8: the quadrotor on 8 intervals (order 8); T3: testfam in one
    basis class; K3: kincar with three linear rows; G4: O4 on per-problem grids"""
    if name in _inputs:
        return _inputs[name]
    if name in ("O4", "O20", "G4"):
        spec = cf.config_O() if name == "O20" else cf.config_O(ninterv=4)
        nb = {"O4": NBIG, "O20": 9, "G4": 5}[name]
        lo, up = cf.obstacle_bounds(nb)
        c = Inputs(name, spec, obstacle_x(spec, nb, 71 if name != "G4" else 61), lo, up, nexact=3)
        if name == "G4":
            scales = np.array([0.5, 1.0, 1.7, 2.0, 3.0])
            c.knots, c.bps = scaled_grids(spec, scales)
            c.x[:, :spec.ncoef[0]] *= scales[:, None]   # x = 8 t on the problem's own horizon
    elif name == "OF5":
        spec = cf.config_OF(3, ninterv=5)
        prm, lo, up = cf.obstacle_field_problems(9, 3)
        c = Inputs(name, spec, field_x(spec, lo, 72), lo, up, prm=prm, nexact=2)
    elif name == "D8":
        spec = cf.config_D(ninterv=8)   # order 8: the KM = 10 instance, rows of degree 10 (thrust^2) and 12 (speed^2)
        lo, up = cf.quadrotor_bounds(5)
        c = Inputs(name, spec, np.random.default_rng(73).standard_normal((5, spec.nC)), lo, up, nexact=2)
    elif name == "T3":
        spec = testfam_spec()
        c = Inputs(name, spec, np.random.default_rng(74).standard_normal((3, spec.nC)), np.full((3, spec.nbounds), -1.0), np.full((3, spec.nbounds), 1.0), nexact=2)
    else:
        spec = rows_spec()
        nb = 7
        kl, ku = cf.kincar_random_bounds(1, nb)
        lo = np.concatenate([kl[:, :6], np.full((nb, 3), -1.0), kl[:, 6:]], axis=1)
        up = np.concatenate([ku[:, :6], np.full((nb, 3), 1.0), ku[:, 6:]], axis=1)
        c = Inputs(name, spec, np.random.default_rng(75).standard_normal((nb, spec.nC)), lo, up, nexact=2)
    c.sl = slack(spec, c.x, c.prm, c.knots)
    c.polys = row_polygons(spec, c.x, c.prm, c.knots)
    # tol = max(1e-9 max |row bound or value|, 64 slack), one figure for the whole case
    fl = flags(spec)
    s0 = spec.nlic
    slots = list(range(s0, s0 + spec.nltc)) + list(range(s0 + spec.nltc + spec.nlfc + spec.nnlic, s0 + spec.nltc + spec.nlfc + spec.nnlic + spec.nnltc))
    big = 0.0
    for r, P in enumerate(c.polys):
        if P is None:
            continue
        big = max(big, float(np.abs(P).max()))
        for bd in (c.lower[:, slots[r]], c.upper[:, slots[r]]):
            big = max(big, float(np.abs(bd[np.abs(bd) < cf.INF_BOUND]).max(initial=0.0)))
    c.tol = max(1e-9 * big, 64.0 * float(c.sl[:, fl == 1].max()))
    _inputs[name] = c
    return c
