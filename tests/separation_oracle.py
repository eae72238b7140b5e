"""ntg_batch_separation's definition (include/ntg_amd.h) for the tests, and the inputs the CPU and GPU tests share.

  deltas         the difference coefficients of every pair, [npairs, ndim, n]: one subtraction each.
  pair_polygons  level-0 polygons of the squared distance in float64: the interval polygons of envelope_oracle on delta, differenced,
                 squared by extrema_oracle.square, summed in dimension order.
  level_sep      the level algorithm (bisect_oracle.levels) at sides = 1 with the threshold rule: a piece is open iff plo < U - tol and not
                 plo >= s2.  Without a threshold (s2 = +inf) it is extrema_oracle.level_oracle at sides = 1.
  slack          2^-39 sum_t S_t^2 with S_t = max_i (|x_a,i| + |x_b,i|) (2 (k - 1) / h_min)^deriv.
  exact_min      the true minimum in fractions.Fraction: extrema_oracle.exact_polygons / exact_extrema on a two-output obstacle-field spec
                 given delta (positions in the plane), the same polynomials summed here for every other case.
"""
import dataclasses
from fractions import Fraction as Fr
from math import inf, isnan, nan

import numpy as np

import bisect_oracle as bo
import envelope_oracle as eo
import envelope_sos_oracle as so
import extrema_oracle as xo
from bisect_oracle import BADPAIR, DEPTH, FULL, NAN, OK   # (the tests take them from here)
from ntg_amd import configs as cf

MAXDIM = 4


def deltas(spec, x, bodies, pairs):
    """[npairs, ndim, n]"""
    sls = eo.coef_slices(spec)
    bodies = np.asarray(bodies)
    return np.stack([np.stack([x[a, sls[bodies[ga, t]]] - x[b, sls[bodies[gb, t]]] for t in range(bodies.shape[1])]) for a, b, ga, gb in np.asarray(pairs)])


def pair_polygons(spec, dl, o0, deriv):
    """[npairs, l, D + 1] from deltas dl; o0: an output of the bodies' basis class"""
    k, m = spec.order[o0], spec.mult[o0]
    S = None
    for t in range(dl.shape[1]):
        P = eo.piece_polygons(spec.knots[o0], k, m, dl[:, t], deriv + 1, 0)[deriv] if deriv < k else np.zeros((dl.shape[0], spec.kninterv[o0], 1))
        G = xo.square(P)
        S = G if S is None else S + G
    return S


def level_sep(polys, kn, tol, s2=inf, max_depth=xo.MAX_DEPTH, cap=xo.CAP):
    """one pair: polys [l][D + 1] floats, kn [l + 1] the breaks.  Returns a dict: min (min_lo, min_hi), when, status, npieces and, for the
    tests, depth (the last level evaluated) and max_open (the most open pieces at a level)"""
    r = bo.levels(bo.POLYGON, [[float(v) for v in B] for B in polys], kn, tol, max_depth, 1, cap, s2)
    return dict(min=r["ext"][:2], when=r["when"][0], status=r["status"], npieces=r["npieces"], depth=r["depth"], max_open=r["max_open"])


def violation(mn, s2):
    """(attained, certified) of the definition"""
    if isnan(s2) or isnan(mn[0]):
        return nan, nan
    return max(s2 - mn[1], 0.0), max(s2 - mn[0], 0.0)


def slack(spec, x, bodies, pairs, deriv):
    """[npairs]"""
    sls = eo.coef_slices(spec)
    bodies = np.asarray(bodies)
    out = np.zeros(len(pairs))
    for q, (a, b, ga, gb) in enumerate(np.asarray(pairs)):
        for t in range(bodies.shape[1]):
            oa, ob = bodies[ga, t], bodies[gb, t]
            hmin = np.diff(np.asarray(spec.knots[oa], dtype=np.float64)).min()
            S = (np.abs(x[a, sls[oa]]) + np.abs(x[b, sls[ob]])).max() * (2.0 * (spec.order[oa] - 1) / hmin) ** deriv
            out[q] += 2.0 ** -39 * S * S
    return out


def exact_polygons(spec, d, o0, deriv):
    """level-0 polygons of ONE pair in Fractions from its delta d [ndim, n]: a list over the intervals of D + 1 Fractions"""
    k, m, l = spec.order[o0], spec.mult[o0], spec.kninterv[o0]
    of = cf.config_OF(1, ninterv=l, order=k)
    if d.shape[0] == 2 and deriv == 0 and m == of.mult[0] and np.array_equal(of.knots[0], spec.knots[o0]):   # positions in the plane: the obstacle-field row, its centre at the origin
        return xo.exact_polygons(of, d.reshape(-1), np.zeros(2))[0]
    t = so.aug_knots(spec.knots[o0], k, m)
    rows = []
    for j in range(l):
        tot = [Fr(0)]
        for c in d:
            p, h = so.interval_poly(t, k, m, c, j, spec.knots[o0])
            for _ in range(deriv):
                p = [v / h for v in so.p_diff(p)]
            tot = so.p_add(tot, so.p_mul(p, p))
        rows.append(so.to_bernstein(tot, 2 * max(k - 1 - deriv, 0)))
    return rows


def exact_min(spec, d, o0, deriv, eps):
    """(lo, hi) floats: lo <= min over the horizon <= hi, hi - lo < eps"""
    lo, hi, _, _ = xo.exact_extrema(exact_polygons(spec, d, o0, deriv), eps)
    return float(lo), float(hi)


# ---------------- the inputs of the tests ----------------
@dataclasses.dataclass
class Inputs:
    name: str
    spec: object
    x: np.ndarray
    bodies: np.ndarray     # [nbody, ndim]
    pairs: np.ndarray      # [npairs, 4] int32
    deriv: int
    sep: float             # the threshold of the case's threshold run
    dl: np.ndarray = None      # deltas
    polys: np.ndarray = None   # pair_polygons
    sl: np.ndarray = None      # slack [npairs]
    tol: float = 0.0

    def kn(self):
        return self.spec.knots[int(self.bodies[0, 0])]

    def levels(self, s2=inf, max_depth=xo.MAX_DEPTH):
        """level_sep of every pair (computed once per setting and kept)"""
        key = (s2, max_depth)
        if key not in self._levels:
            self._levels[key] = [level_sep(P, self.kn(), self.tol, s2, max_depth) for P in self.polys]
        return self._levels[key]

    _levels: dict = dataclasses.field(default_factory=dict)


NBIG = 67   # leaves the persistent loop a partial last pass
CASES = [("S4", 0), ("S20", 0), ("Q8", 0), ("Q8", 1)]
_inputs = {}


def inputs(name, deriv=0):
    """S4 / S20: three cars per problem on 4 / 20 knot intervals, 67 / 9 problems, three pairs per problem (two cars of the problem, and two
    pairs across problems); Q8: the quadrotor's position on 8 intervals (order 8), all pairs of 5 problems"""
    if (name, deriv) in _inputs:
        return _inputs[(name, deriv)]
    if name in ("S4", "S20"):
        l, nbps, nb = (4, 21, NBIG) if name == "S4" else (20, 101, 9)
        spec = cf._kincar_spec(3, 6, 3, l, nbps, 5.0, f"kincar-6out-k6-l{l}")
        gv = xo.greville(spec)
        rng = np.random.default_rng(81)
        cols = []
        for c in range(3):
            cols.append(8.0 * gv + rng.standard_normal((nb, gv.size)))
            cols.append(3.0 * (c - 1) + rng.standard_normal((nb, gv.size)))
        x = np.concatenate(cols, axis=1)
        bodies = np.array([[0, 1], [2, 3], [4, 5]], dtype=np.int32)
        pairs = np.array([p for a in range(nb) for p in ((a, a, 0, 1), (a, (7 * a + 3) % nb, 0, 2), (a, (5 * a + 1) % nb, 1, 1))], dtype=np.int32)
        sep = 2.0
    else:
        spec = cf.config_D(ninterv=8)
        x = np.random.default_rng(83).standard_normal((5, spec.nC))
        bodies = np.array([[0, 1, 2]], dtype=np.int32)
        pairs = np.array([(a, b, 0, 0) for a in range(5) for b in range(a + 1, 5)], dtype=np.int32)
        sep = 1.0
    c = Inputs(name, spec, x, bodies, pairs, deriv, sep)
    c.dl = deltas(spec, x, bodies, pairs)
    c.polys = pair_polygons(spec, c.dl, int(bodies[0, 0]), deriv)
    c.sl = slack(spec, x, bodies, pairs, deriv)
    c.tol = max(1e-9 * float(np.abs(c.polys).max()), 64.0 * float(c.sl.max()))
    _inputs[(name, deriv)] = c
    return c
