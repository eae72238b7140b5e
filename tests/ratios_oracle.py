"""ntg_batch_ratios's definition (include/ntg_amd.h) for the tests, and the inputs the CPU and GPU tests share.

  pair_polygons   level-0 pairs of every ratio in float64: forms_oracle.form_polygons of the forms, each side the chain of
                  forms_oracle.product (the chain so far times the next form), the lower side raised by envelope_oracle.elevate.
  level_oracle    the level algorithm (bisect_oracle.levels) on pairs, with the pair rule -- quotients of the points where every denominator
                  point is positive, (-inf, +inf) otherwise; an end with denominator <= 0 stops the loop: POLE.  It records how far every
                  decision was from its limit (margin), the smallest denominator point and the largest quotient of the retired pieces.
  exact_extrema   the true minimum and maximum of a ratio in exact arithmetic: forms_oracle.exact_polygons multiplied and elevated in Fractions,
                  then bisected on integers (both polygons of a pair scaled alike) until the enclosure is narrower than eps.
  slack           the header's rounding statement: eps_side = prod m_f (sum delta_f / m_f + 2^-43), (eps_N + |rho| eps_D) / (d_min - eps_D).

A ratio is a pair (num, den) of lists of form indices (ntg_amd.forms.ratio).  Shapes are small: each case is the smallest at which its path
can still go wrong.
"""
import dataclasses
from fractions import Fraction as Fr
from math import comb, inf, isnan, nan

import numpy as np

import bisect_oracle as bo
import envelope_oracle as eo
import extrema_oracle as xo
import forms_oracle as fo
from bisect_oracle import DEPTH, FULL, NAN, OK, POLE, violation   # (the tests take them from here)
from cert_common import scaled_grids
from ntg_amd import configs as cf, forms as fm

MAXDEG = 24
# Every case runs at two tolerances per ratio.  `tol`, in slacks of its worst problem: there every decision of the oracle stays 16 slacks of
# its own problem away from its limit (tests/test_ratios_oracle.py), so equal status and npieces follow from the rounding statement alone; a
# piece that retires lies within tol of U or V, so tol must be many such windows wide for a seed to exist with 24 problems x 4 ratios.  That
# tolerance is coarse (kappa^2: up to 8 % of a problem's peak on RK4, 59 % on RK20, above the peak of the slowest-turning cars of RPP, R8 and
# RMOD; the bisection stops after 5 to 13 levels).  `fine`, 1e-9 of the ratio's largest quotient: up to 26 levels, up to 47 pairs open at
# once; the decisions' margins are then far below the slack (1e-8 to 1e-5 of it), and that the kernel decides alike is asserted, not implied.
TOL_SLACKS = 1024.0


# ---------------- level 0 ----------------
def ratio_shape(spec, forms, ratio):
    """(output whose knot intervals the ratio has, dN, dD)"""
    shapes = [fo.shape(spec, forms[f]) for f in ratio[0] + ratio[1]]
    return shapes[0][0], sum(fo.shape(spec, forms[f])[1] for f in ratio[0]), sum(fo.shape(spec, forms[f])[1] for f in ratio[1])


def side_polygon(F, idx, nb, l):
    """the chain G = F[idx[0]]; G = G (x) F[idx[a]]: [nb, l, d + 1]; an empty side is the point 1"""
    if not idx:
        return np.ones((nb, l, 1))
    G = F[idx[0]]
    for f in idx[1:]:
        G = fo.product(G, F[f])
    return G


def pair_polygons(spec, x, forms, ratios, fprm=None, knots=None):
    """per ratio (N, Q), each [nb, l, DR + 1]"""
    F = fo.form_polygons(spec, x, forms, fprm, knots)
    out = []
    for num, den in ratios:
        nb, l = F[(num + den)[0]].shape[:2]
        N, Q = side_polygon(F, num, nb, l), side_polygon(F, den, nb, l)
        while N.shape[-1] < Q.shape[-1]:
            N = eo.elevate(N)
        while Q.shape[-1] < N.shape[-1]:
            Q = eo.elevate(Q)
        out.append((N, Q))
    return out


# ---------------- the definition ----------------
def _quotients(P):
    """(plo, phi) of a pair"""
    N, Q = P
    if any(isnan(v) for v in N) or any(isnan(v) for v in Q):
        return nan, nan
    if all(d > 0.0 for d in Q):
        rho = [n / d for n, d in zip(N, Q)]
        return min(rho), max(rho)
    return -inf, inf


def _end_quotients(P):
    """the quotients at the two ends; a denominator <= 0 there is a pole, a NaN there is never taken"""
    N, Q = P
    return [(None if d <= 0.0 else n / d, 0, inf) for n, d in ((N[0], Q[0]), (N[-1], Q[-1]))]


PAIR = (_end_quotients, _quotients, lambda P: tuple(zip(bo.halve(P[0]), bo.halve(P[1]))))   # pieces: (N, Q), lists of floats


def level_oracle(N0, Q0, kn, tol, max_depth=xo.MAX_DEPTH, sides=3, cap=xo.CAP):
    """one ratio of one problem: N0, Q0 [l][DR + 1] floats, kn [l + 1] its breaks.  bisect_oracle.levels on pairs: its dict (margin over every
    decision made with a finite plo / phi), and dmin (the smallest denominator point of the retired pieces) and rmax (the largest
    |quotient| of the retired pieces and the ends taken)"""
    dmin = [inf]

    def retired(P):
        dmin[0] = min(dmin[0], min(P[1]))

    r = bo.levels(PAIR, [([float(v) for v in N], [float(v) for v in Q]) for N, Q in zip(N0, Q0)], kn, tol, max_depth, sides, cap, retired=retired)
    r.update(dmin=dmin[0], rmax=nan if r["status"] == NAN else inf if r["status"] == POLE else max(abs(v) for v in r["ext"]))
    return r


# ---------------- exact arithmetic ----------------
def _bern_mul(P, Q):
    d, e = len(P) - 1, len(Q) - 1
    G = [Fr(0)] * (d + e + 1)
    for i in range(d + 1):
        for j in range(e + 1):
            G[i + j] += Fr(comb(d, i) * comb(e, j), comb(d + e, i + j)) * P[i] * Q[j]
    return G


def _bern_elevate(B, D):
    while len(B) - 1 < D:
        d = len(B) - 1
        B = [B[0]] + [Fr(i, d + 1) * B[i - 1] + (1 - Fr(i, d + 1)) * B[i] for i in range(1, d + 1)] + [B[d]]
    return B


def exact_pairs(spec, xb, forms, ratio, fb=None, kb=None):
    """level-0 pairs of ONE problem and one ratio in Fractions: a list over the intervals of (N, Q), DR + 1 Fractions each"""
    ex = fo.exact_polygons(spec, xb, forms, fb, kb)
    num, den = ratio
    out = []
    for j in range(len(ex[(num + den)[0]])):
        sides = []
        for idx in (num, den):
            G = [Fr(1)]
            for a, f in enumerate(idx):
                G = list(ex[f][j]) if a == 0 else _bern_mul(G, ex[f][j])
            sides.append(G)
        D = max(len(sides[0]), len(sides[1])) - 1
        out.append((_bern_elevate(sides[0], D), _bern_elevate(sides[1], D)))
    return out


def _ints(B):
    """(integers, c) with B = integers / c"""
    c = 1
    for v in B:
        c = c * v.denominator // _gcd(c, v.denominator)
    return [int(v * c) for v in B], c


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def _split_ints(B):
    """both halves of an integer polygon, scaled by 2^D alike"""
    D = len(B) - 1
    R, L = list(B), [B[0] << D]
    for r in range(1, D + 1):
        for s in range(D + 1 - r):
            R[s] = R[s] + R[s + 1]
        L.append(R[0] << (D - r))
    return L, [R[s] << s for s in range(D + 1)]


def _exact_min(pairs, eps):
    """(lo, hi), Fractions with lo <= min over the horizon <= hi and hi - lo < eps; hi is attained.  The denominator must be positive at
    every end visited"""
    pieces = []
    for N, Q in pairs:
        (n, cn), (q, cq) = _ints(N), _ints(Q)
        pieces.append((n, q, Fr(cq, cn)))
    quot = lambda n, q, c: Fr(n, q) * c
    for n, q, c in pieces:
        assert q[0] > 0 and q[-1] > 0, "a pole"
    U = min(min(quot(n[0], q[0], c), quot(n[-1], q[-1], c)) for n, q, c in pieces)
    while True:
        keep, lo = [], U
        for n, q, c in pieces:
            pos = all(d > 0 for d in q)
            plo = min(quot(a, d, c) for a, d in zip(n, q)) if pos else None
            if not pos or plo < U:
                keep.append((n, q, c))
                lo = None if (lo is None or not pos) else min(lo, plo)
        if lo is not None and U - lo < eps:
            return lo, U
        nxt = []
        for n, q, c in keep:
            (nl, nr), (ql, qr) = _split_ints(n), _split_ints(q)
            assert qr[0] > 0, "a pole"
            U = min(U, quot(nr[0], qr[0], c))
            nxt += [(nl, ql, c), (nr, qr, c)]
        pieces = nxt


def exact_extrema(spec, xb, forms, ratio, eps, fb=None, kb=None):
    """(min_lo, min_hi, max_lo, max_hi) of one ratio of one problem in Fractions, each enclosure narrower than eps"""
    pairs = exact_pairs(spec, xb, forms, ratio, fb, kb)
    eps = Fr(float(eps))
    lo, hi = _exact_min(pairs, eps)
    nlo, nhi = _exact_min([([-v for v in N], Q) for N, Q in pairs], eps)
    return lo, hi, -nhi, -nlo


# ---------------- the rounding statement ----------------
def side_eps(c, idx):
    """[nb]: eps_side = prod m_f (sum delta_f / m_f + 2^-43), delta_f = the form's slack, m_f = delta_f + the largest |point| of its polygons"""
    nb = c.x.shape[0]
    prod, rel = np.ones(nb), np.full(nb, 2.0 ** -43)
    for f in idx:
        delta = c.fsl[:, f]
        m = delta + np.abs(c.fpolys[f]).reshape(nb, -1).max(axis=1)
        prod, rel = prod * m, rel + delta / m
    return prod * rel


def slack_of(c, b, r, rmax, dmin):
    """(eps_N + |rho| eps_D) / (d_min - eps_D); inf where no certificate is claimed"""
    eN, eD = side_eps(c, c.ratios[r][0])[b], side_eps(c, c.ratios[r][1])[b]
    if not (dmin > eD) or not np.isfinite(rmax):
        return inf
    return float((eN + rmax * eD) / (dmin - eD))


def values(spec, z, forms, ratios, fprm=None):
    """the ratios from flag values z [nb, nt, nz] in double precision: [nb, nt, nratio]"""
    v = fo.values(spec, z, forms, fprm)
    out = np.empty(v.shape[:2] + (len(ratios),))
    for r, (num, den) in enumerate(ratios):
        out[:, :, r] = np.prod(v[:, :, num], axis=2) / np.prod(v[:, :, den], axis=2)
    return out


# ---------------- the inputs of the tests ----------------
@dataclasses.dataclass
class Inputs:
    name: str
    spec: object
    x: np.ndarray
    forms: list
    ratios: list
    fprm: object = None
    knots: object = None
    bps: object = None
    nexact: int = 1
    tol: np.ndarray = None    # [nratio]: every ratio has its own unit
    fine: np.ndarray = None   # [nratio]: 1e-9 of the ratio's largest quotient
    sl: np.ndarray = None     # slack [nb, nratio]
    fsl: np.ndarray = None    # the forms' slack [nb, nform]
    fpolys: list = None       # forms_oracle.form_polygons
    pairs: list = None        # pair_polygons
    _levels: dict = dataclasses.field(default_factory=dict)

    def kn(self, b, r):
        return self.spec.knots[ratio_shape(self.spec, self.forms, self.ratios[r])[0]] if self.knots is None else self.knots[b]

    def levels(self, tol=None, max_depth=xo.MAX_DEPTH, sides=3):
        """level_oracle of every (problem, ratio): [nb][nratio] dicts (computed once per setting and kept).  tol: one figure for every ratio;
        an array: one per ratio; None: the case's own tolerance of each ratio"""
        tols = tuple(self.tol if tol is None else [float(t) for t in tol] if np.ndim(tol) else [tol] * len(self.ratios))
        key = (tols, max_depth, sides)
        if key not in self._levels:
            self._levels[key] = [[level_oracle(N[b], Q[b], self.kn(b, r), tols[r], max_depth, sides) for r, (N, Q) in enumerate(self.pairs)] for b in range(self.x.shape[0])]
        return self._levels[key]

    def finish(self):
        """the polygons, the slack (from a first run at 1e-6 of the largest end quotient: the statement needs the retired pieces) and the
        tolerance of every ratio: max(1e-9 of its largest quotient, TOL_SLACKS slacks)"""
        self.fsl = fo.slack(self.spec, self.x, self.forms, self.fprm, self.knots)
        self.fpolys = fo.form_polygons(self.spec, self.x, self.forms, self.fprm, self.knots)
        self.pairs = pair_polygons(self.spec, self.x, self.forms, self.ratios, self.fprm, self.knots)
        nb, nr = self.x.shape[0], len(self.ratios)
        self.sl, self.tol, self.fine = np.empty((nb, nr)), np.empty(nr), np.empty(nr)
        for r, (N, Q) in enumerate(self.pairs):
            ends = max(abs(n / d) for n, d in zip(N[:, :, (0, -1)].reshape(-1), Q[:, :, (0, -1)].reshape(-1)) if d > 0.0)
            first = [level_oracle(N[b], Q[b], self.kn(b, r), 1e-6 * ends) for b in range(nb)]
            self.sl[:, r] = [slack_of(self, b, r, first[b]["rmax"], first[b]["dmin"]) for b in range(nb)]
            self.fine[r] = 1e-9 * max(f["rmax"] for f in first)
            self.tol[r] = max(self.fine[r], TOL_SLACKS * float(self.sl[:, r].max()))
        return self


def kincar_forms(spec):
    """S = x'^2 + y'^2, T = x' y'' - y' x'', x', y'"""
    return [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1)), fm.linear(fm.entry(spec, 0, 1), 1.0), fm.linear(fm.entry(spec, 1, 1), 1.0)]


KAPPA2, LAT2, SLOPE, S2 = fm.ratio([1, 1], [0, 0, 0]), fm.ratio([1, 1], [0]), fm.ratio([3], [2]), fm.ratio([0, 0])
# The seeds are chosen so that every decision of the float64 oracle keeps 16 slacks from its limit: tests/test_ratios_oracle.py
SEEDS = {"RK4": 1, "RK20": 1, "RPP": 1, "R8": 5, "RMOD": 1}
CASES = ["RK4", "RK20", "RPP", "R8", "RMOD"]
EXACT_CASES = ["RK4", "RK20", "RPP", "R8"]
_inputs = {}


def inputs(name, family=0):
    """RK4 / RK20 / RPP: forms_oracle's K4 / K20 / PP cars with the ratios of the kinematic car; R8: the quadrotor plan of order 8, one ratio
    of degree 20; RMOD: the unicycle module's plan"""
    if name in _inputs:
        return _inputs[name]
    if name in ("RK4", "RK20", "RPP"):
        l = 20 if name == "RK20" else 4
        spec = cf._kincar_spec(1, 6, 3, l, 5 * l + 1, 5.0, f"kincar-2out-k6-l{l}")
        nb = {"RK4": 24, "RK20": 8, "RPP": 12}[name]
        x = fo.kincar_x(spec, nb, SEEDS[name], *((0.1, 0.3) if name == "RK20" else (0.2, 1.5)))   # (x' stays positive: y' / x' has no pole)
        c = Inputs(name, spec, x, kincar_forms(spec), {"RK4": [KAPPA2, LAT2, SLOPE, S2], "RK20": [KAPPA2], "RPP": [KAPPA2, LAT2]}[name])
        if name == "RPP":
            scales = np.linspace(0.5, 2.0, nb)
            c.knots, c.bps = scaled_grids(spec, scales)
            c.x[:, :spec.ncoef[0]] *= scales[:, None]
    elif name == "R8":
        spec = cf.config_D(ninterv=8)   # order 8: the KM = 10 instances
        e = lambda o, r: fm.entry(spec, o, r)
        forms = [fm.square(e(0, 2)) + fm.square(e(1, 2)) + fm.square(e(2, 2), shift=-9.81, w=4.0),      # degree 10
                 fm.product(e(0, 1), e(1, 3)) + fm.product(e(1, 1), e(0, 3), w=-1.0)]                    # degree 10
        c = Inputs(name, spec, 0.05 * np.random.default_rng(SEEDS[name]).standard_normal((6, spec.nC)), forms, [fm.ratio([1, 1], [0, 0])])   # (near hover: the thrust form stays positive)
    else:
        spec = fo.module_spec(family)
        c = Inputs(name, spec, np.random.default_rng(SEEDS[name]).standard_normal((8, spec.nC)), [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1))],
                   [fm.ratio([1], [0]), fm.ratio([0, 0])])
    _inputs[name] = c.finish()
    return c


NAN_RATIOS = [KAPPA2, SLOPE, fm.ratio([2]), fm.ratio([2, 2], [2])]   # the last two name x' alone


def parked_x(c):
    """RK4's x with problem 7 standing still on knot interval 1 (its six coefficients there equal, of x and of y): a pole where the ratio has
    a denominator"""
    xp, n = c.x.copy(), c.spec.ncoef[0]
    xp[7, 3:9] = xp[7, 3]; xp[7, n + 3:n + 9] = xp[7, n + 3]
    return xp


def nan_x(c):
    """RK4's x with a NaN coefficient of y on the first knot interval of problem 5: of NAN_RATIOS the first two name y"""
    xn = c.x.copy()
    xn[5, c.spec.ncoef[0] + 1] = np.nan
    return xn
