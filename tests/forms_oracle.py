"""ntg_batch_forms's definition (include/ntg_amd.h) for the tests, and the inputs the CPU and GPU tests share.

  product         the Bezier product of two polygons of degrees d and e in float64: g_m = sum_{i + j = m} W_{d,e}[i][j] p_i q_j, i ascending.
  form_polygons   level-0 polygons of every form: the interval polygons of envelope_oracle, differenced, shifted, multiplied, weighted,
                  elevated and summed in declared order.  The levels are extrema_oracle.level_oracle: bisect_oracle.levels on single polygons.
  exact_polygons  the same polynomials in fractions.Fraction through envelope_sos_oracle's rational machinery (de Boor's recursion on
                  polynomials, power basis, one conversion to the Bernstein basis at the form's degree), extended here to products;
                  extrema_oracle.exact_extrema then gives the true minimum and maximum.
  slack           2^-39 sum_t |w_t| S_u S_v, S_x = max_i |c_{o,i}| (2 (k - 1) / h_min)^r + |shift|, S_v = 1 for a linear term.

A form is a list of ntg_amd.forms.Term.  Shapes are small: each case is the smallest at which its path can still go wrong.
"""
import dataclasses
from fractions import Fraction as Fr
from math import comb

import numpy as np

import envelope_oracle as eo
import envelope_sos_oracle as so
import extrema_oracle as xo
from bisect_oracle import DEPTH, FULL, NAN, OK, violation   # (the tests take them from here)
from cert_common import full_list_problem, greville, scaled_grids
from ntg_amd import configs as cf, forms as fm



def product(P, Q):
    """Bezier product of the polygons P [..., d + 1] and Q [..., e + 1]: [..., d + e + 1]"""
    d, e = P.shape[-1] - 1, Q.shape[-1] - 1
    G = np.zeros(np.broadcast_shapes(P.shape[:-1], Q.shape[:-1]) + (d + e + 1,))
    for i in range(d + 1):
        for j in range(e + 1):
            G[..., i + j] += comb(d, i) * comb(e, j) / comb(d + e, i + j) * P[..., i] * Q[..., j]
    return G


def shape(spec, form):
    """(output whose knot intervals the form has, degree D of its polygon); raises if the form names two basis classes"""
    D, o0 = 0, None
    for t in form:
        o, r = so.entry_of(spec, t.u)
        deg = max(spec.order[o] - 1 - r, 0)
        outs = [o]
        if t.v >= 0:
            ov, rv = so.entry_of(spec, t.v)
            deg += max(spec.order[ov] - 1 - rv, 0)
            outs.append(ov)
        o0 = outs[0] if o0 is None else o0
        assert all(so.same_class(spec, q, o0) for q in outs), "the form names outputs of different basis classes"
        D = max(D, deg)
    return o0, D


def _shift(c, p, fprm):
    """[nb] or a scalar"""
    return c + (fprm[:, p] if p >= 0 else 0.0)


def form_polygons(spec, x, forms, fprm=None, knots=None):
    """level-0 polygons in float64: per form [nb, l, D + 1].  knots [nb, l + 1]: every problem's own breaks"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb = x.shape[0]
    sls = eo.coef_slices(spec)
    cache = {}

    def polys(v, c, p):
        o, r = so.entry_of(spec, v)
        if o not in cache:
            if knots is None:
                cache[o] = eo.piece_polygons(spec.knots[o], spec.order[o], spec.mult[o], x[:, sls[o]], spec.maxderiv[o], 0)
            else:
                per = [eo.piece_polygons(knots[b], spec.order[o], spec.mult[o], x[b:b + 1, sls[o]], spec.maxderiv[o], 0) for b in range(nb)]
                cache[o] = [np.concatenate([q[i] for q in per], axis=0) for i in range(len(per[0]))]
        P = cache[o][r] if r < spec.order[o] else np.zeros((nb, spec.kninterv[o], 1))
        return P - np.broadcast_to(_shift(c, p, fprm), (nb,))[:, None, None]

    out = []
    for form in forms:
        o0, D = shape(spec, form)
        S = np.zeros((nb, spec.kninterv[o0], D + 1))
        for t in form:
            G = polys(t.u, t.su, t.pu)
            if t.v >= 0:
                G = product(G, polys(t.v, t.sv, t.pv))
            G = t.w * G
            while G.shape[-1] - 1 < D:
                G = eo.elevate(G)
            S = S + G
        out.append(S)
    return out


def exact_polygons(spec, xb, forms, fb=None, kb=None):
    """level-0 polygons of ONE problem in Fractions: per form a list over the intervals of D + 1 Fractions"""
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])
    cache = {}

    def factor(v, c, p, j):
        o, r = so.entry_of(spec, v)
        if (o, j) not in cache:
            brk = spec.knots[o] if kb is None else kb
            cache[(o, j)] = so.interval_poly(so.aug_knots(brk, spec.order[o], spec.mult[o]), spec.order[o], spec.mult[o], xb[off[o]:off[o + 1]], j, brk)
        q, h = cache[(o, j)]
        for _ in range(r):
            q = [a / h for a in so.p_diff(q)]
        return so.p_add(q, [-(Fr(float(c)) + (Fr(float(fb[p])) if p >= 0 else 0))])

    out = []
    for form in forms:
        o0, D = shape(spec, form)
        rows = []
        for j in range(spec.kninterv[o0]):
            tot = [Fr(0)]
            for t in form:
                q = factor(t.u, t.su, t.pu, j)
                if t.v >= 0:
                    q = so.p_mul(q, factor(t.v, t.sv, t.pv, j))
                tot = so.p_add(tot, [Fr(float(t.w)) * a for a in q])
            rows.append(so.to_bernstein(tot, D))
        out.append(rows)
    return out


def exact_extrema(spec, xb, forms, eps, fb=None, kb=None):
    """per form (min_lo, min_hi, max_lo, max_hi) in Fractions, each enclosure narrower than eps[f]: extrema_oracle's rational bisection on
    the exact polygons of the products"""
    return [xo.exact_extrema(P, eps[f]) for f, P in enumerate(exact_polygons(spec, xb, forms, fb, kb))]


def slack(spec, x, forms, fprm=None, knots=None):
    """[nb, nform]"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])

    def S(v, c, p):
        o, r = so.entry_of(spec, v)
        hmin = np.diff(np.asarray(spec.knots[o], dtype=np.float64)).min() if knots is None else np.diff(np.asarray(knots), axis=1).min(axis=1)
        return np.abs(x[:, off[o]:off[o + 1]]).max(axis=1) * (2.0 * (spec.order[o] - 1) / hmin) ** r + np.abs(_shift(c, p, fprm))

    out = np.zeros((x.shape[0], len(forms)))
    for f, form in enumerate(forms):
        for t in form:
            out[:, f] += 2.0 ** -39 * abs(t.w) * S(t.u, t.su, t.pu) * (S(t.v, t.sv, t.pv) if t.v >= 0 else 1.0)
    return out


def values(spec, z, forms, fprm=None):
    """the forms from flag values z [nb, nt, nz] in double precision: [nb, nt, nform]"""
    z = np.asarray(z, dtype=np.float64)
    out = np.zeros(z.shape[:2] + (len(forms),))
    for f, form in enumerate(forms):
        for t in form:
            g = z[:, :, t.u] - np.reshape(_shift(t.su, t.pu, fprm) * np.ones(z.shape[0]), (-1, 1))
            if t.v >= 0:
                g = g * (z[:, :, t.v] - np.reshape(_shift(t.sv, t.pv, fprm) * np.ones(z.shape[0]), (-1, 1)))
            out[:, :, f] += t.w * g
    return out


def decision_margin(polys, kn, tol, max_depth=xo.MAX_DEPTH, sides=3):
    """(the smallest |plo - (U - tol)| or |phi - (V + tol)| over every decision level_oracle makes, its result)"""
    r = xo.level_oracle(polys, kn, tol, max_depth, sides)
    return r["margin"], r


# ---------------- the inputs of the tests ----------------
@dataclasses.dataclass
class Inputs:
    name: str
    spec: object
    x: np.ndarray
    forms: list
    fprm: object = None
    knots: object = None    # [nb, l + 1]: per-problem grids
    bps: object = None
    nexact: int = 2
    expect: int = OK        # the status every form ends with at the case's tolerance
    tol: float = 0.0
    sl: np.ndarray = None   # slack [nb, nform]
    polys: list = None      # form_polygons
    _levels: dict = dataclasses.field(default_factory=dict)

    def kn(self, b, f):
        return self.spec.knots[shape(self.spec, self.forms[f])[0]] if self.knots is None else self.knots[b]

    def levels(self, tol=None, max_depth=xo.MAX_DEPTH, sides=3):
        """level_oracle of every (problem, form): [nb][nform] dicts (computed once per setting and kept)"""
        tol = self.tol if tol is None else tol
        key = (tol, max_depth, sides)
        if key not in self._levels:
            self._levels[key] = [[xo.level_oracle(self.polys[f][b], self.kn(b, f), tol, max_depth, sides) for f in range(len(self.forms))] for b in range(self.x.shape[0])]
        return self._levels[key]


def kincar_x(spec, nb, seed, ax=0.6, ay=1.5):
    """cars that drive along +x at about 8 m/s and weave: x = 8 t and y = 0.5, both perturbed (cert_common.obstacle_x's shape)"""
    rng = np.random.default_rng(seed)
    gv = greville(spec) * (5.0 / spec.knots[0][-1])
    return np.concatenate([8.0 * gv[None, :] + ax * rng.standard_normal((nb, gv.size)), 0.5 + ay * rng.standard_normal((nb, gv.size))], axis=1)


def kincar_forms(spec, full):
    e = lambda o, r: fm.entry(spec, o, r)
    forms = [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1))]
    if full:
        forms += [fm.product(e(0, 1), e(0, 2)) + fm.product(e(1, 1), e(1, 2)),                  # v . a
                  fm.linear(e(0, 0), 0.6) + fm.linear(e(1, 0), 0.8, param=0),                   # 0.6 x + 0.8 (y - fprm[0]): a half plane
                  fm.ellipse(spec, 0, 1, 2.0, 3.0, 1, 2),                                       # centre fprm[1:3], weights 1/4 and 1/9
                  fm.square(e(0, 0)) + fm.product(e(0, 1), e(1, 2))]                            # x^2 + x' y'': a term below the form's degree
    return forms


# The seeds (and K4's horizon) are chosen so that every decision of the float64 oracle keeps 16 slacks from its limit: tests/test_forms_oracle.py
SEEDS = {"K4": 381, "K20": 105, "PP": 93, "D8": 107, "T4": 96, "MOD": 97}
HORIZON = {"K4": 5.0, "K20": 5.0, "PP": 5.0}
CASES = ["K4", "K20", "L80", "D8", "T4", "MOD", "PP"]
EXACT_CASES = [c for c in CASES if c != "MOD"]
_inputs = {}


def module_spec(family=0):
    """the plan of the in-tree unicycle module (ntg_amd/modules/unicycle.hip); `family` is the id ntg_family_load gave it"""
    return cf.config_U(family)


def inputs(name, family=0):
    if name in _inputs:
        return _inputs[name]
    if name in ("K4", "K20", "PP"):
        l = 20 if name == "K20" else 4
        spec = cf._kincar_spec(1, 6, 3, l, 5 * l + 1, HORIZON[name], f"kincar-2out-k6-l{l}")
        nb = {"K4": 24, "K20": 8, "PP": 12}[name]
        c = Inputs(name, spec, kincar_x(spec, nb, SEEDS[name], *((0.1, 0.3) if name == "K20" else ())), kincar_forms(spec, name == "K4"))
        if name == "K4":
            rng = np.random.default_rng(SEEDS[name] + 1000)
            c.fprm = np.stack([rng.uniform(-1.0, 1.0, nb), rng.uniform(10.0, 30.0, nb), rng.uniform(-2.0, 2.0, nb)], axis=1)
        if name == "PP":
            scales = np.linspace(0.5, 2.0, nb)
            c.knots, c.bps = scaled_grids(spec, scales)
            c.x[:, :spec.ncoef[0]] *= scales[:, None]   # x = 8 t on the problem's own horizon
    elif name == "L80":
        spec, x = full_list_problem()
        y = fm.entry(spec, 1, 0)
        c = Inputs(name, spec, np.repeat(x, 2, axis=0), [fm.linear(y, 1.0), fm.product(y, y, pu=-1, pv=0)], fprm=np.zeros((2, 1)), nexact=1, expect=FULL)   # all 80 intervals open at level 0
        c.x[1, spec.ncoef[0]:] *= 0.5
    elif name == "D8":
        spec = cf.config_D(ninterv=8)   # order 8: the KM = 10 instances
        e = lambda o, r: fm.entry(spec, o, r)
        forms = [fm.square(e(0, 2)) + fm.square(e(1, 2)) + fm.square(e(2, 2), shift=-9.81, w=4.0),
                 fm.product(e(0, 1), e(1, 3)) + fm.product(e(1, 1), e(0, 3), w=-1.0)]
        c = Inputs(name, spec, np.random.default_rng(SEEDS[name]).standard_normal((6, spec.nC)), forms)
    elif name == "T4":
        spec = cf.config_T(nout=3, order=5, ninterv=4)   # outputs 0, 1 in one basis class, output 2 in another
        e = lambda o, r: fm.entry(spec, o, r)
        forms = [fm.product(e(0, 0), e(1, 1)) + fm.linear(e(0, 2), 0.5), fm.square(e(2, 0), shift=0.25) + fm.product(e(2, 1), e(2, 2), w=-2.0)]
        c = Inputs(name, spec, np.random.default_rng(SEEDS[name]).standard_normal((4, spec.nC)), forms)
    else:
        spec = module_spec(family)
        e = lambda o, r: fm.entry(spec, o, r)
        c = Inputs(name, spec, np.random.default_rng(SEEDS[name]).standard_normal((8, spec.nC)), [fm.speed2(spec, (0, 1)), fm.cross(spec, (0, 1), (1, 1))])
    c.sl = slack(spec, c.x, c.forms, c.fprm, c.knots)
    c.polys = form_polygons(spec, c.x, c.forms, c.fprm, c.knots)
    c.tol = max(1e-9 * max(float(np.abs(P).max()) for P in c.polys), 64.0 * float(c.sl.max()))
    _inputs[name] = c
    return c


def cross_class_form(spec):
    """T4's refusal: a form across the two basis classes of config_T"""
    return fm.product(fm.entry(spec, 0, 0), fm.entry(spec, 2, 0))
