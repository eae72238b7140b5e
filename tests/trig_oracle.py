"""ntg_batch_trig's definition (include/ntg_amd.h) for the tests, decision by decision in float64, and the inputs the CPU and GPU tests share.

  pieces0   level-0 pieces of every form: per term the entries' interval polygons of envelope_oracle, differenced, times coef, elevated,
            summed, the phase added; the LIN terms' weighted polygons summed into one (rule 1).
  levels    the level loop of ntg_batch_extrema (bisect_oracle.levels) on those pieces with the enclosure of rule 2 and the ends of rule 3.
            It records the depth, the most pieces open at a level, and the smallest margin of any open / retire decision.
  slack     2^-39 sum_t |w_t| (1 + A_t), A_t = |phase| + |fprm[pp]| + sum_i |coef_i| S_i, S_i as in forms_oracle; a term with A_t > 2^11 adds
            2^-51 |w_t| A_t^2.
  values    the forms from flag values, for the sampled extrema.

A form is a list of ntg_amd.trig.Term.  Shapes are small: each case is the smallest at which its path can still go wrong.
"""
import dataclasses
from math import inf, nan

import numpy as np

import bisect_oracle as bo
import envelope_oracle as eo
import envelope_sos_oracle as so
from bisect_oracle import CAP, DEPTH, FULL, MAX_DEPTH, NAN, OK, violation   # (the tests take them from here)
from cert_common import full_list_problem, scaled_grids
from ntg_amd import configs as cf, trig as tg

SIN, COS, LIN = tg.SIN, tg.COS, tg.LIN


def shape(spec, form):
    """(output whose knot intervals the form has, degree D of its polygons); raises if the form names two basis classes"""
    D, o0 = 0, None
    for t in form:
        for v in t.ent:
            o, r = so.entry_of(spec, v)
            o0 = o if o0 is None else o0
            assert so.same_class(spec, o, o0), "the form names outputs of different basis classes"
            D = max(D, max(spec.order[o] - 1 - r, 0))
    return o0, D


def _param(t, fprm, nb):
    return np.zeros(nb) if t.pp < 0 else np.asarray(fprm, dtype=np.float64)[:, t.pp]


def pieces0(spec, x, forms, fprm=None, knots=None):
    """per form (meta, P): meta = ([(kind, w) of the SIN / COS terms in declared order], has a LIN polygon, W); P [nb, l, np, D + 1], the
    terms' angle polygons and behind them the LIN terms' polygon"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb = x.shape[0]
    sls = eo.coef_slices(spec)
    cache = {}

    def entry_poly(v):
        o, r = so.entry_of(spec, v)
        if o not in cache:
            if knots is None:
                cache[o] = eo.piece_polygons(spec.knots[o], spec.order[o], spec.mult[o], x[:, sls[o]], spec.maxderiv[o], 0)
            else:
                per = [eo.piece_polygons(knots[b], spec.order[o], spec.mult[o], x[b:b + 1, sls[o]], spec.maxderiv[o], 0) for b in range(nb)]
                cache[o] = [np.concatenate([q[i] for q in per], axis=0) for i in range(len(per[0]))]
        return cache[o][r] if r < spec.order[o] else np.zeros((nb, spec.kninterv[o], 1))

    def angle(t, deg):
        S = 0.0
        for v, c in zip(t.ent, t.coef):
            G = np.float64(c) * entry_poly(v)
            while G.shape[-1] - 1 < deg:
                G = eo.elevate(G)
            S = S + G
        return S + (np.float64(t.phase) + _param(t, fprm, nb))[:, None, None]

    out = []
    for form in forms:
        o0, D = shape(spec, form)
        trig = [t for t in form if t.kind != LIN]
        polys = [angle(t, D) for t in trig]
        lam = None
        for t in form:
            if t.kind != LIN:
                continue
            dt = max(max(spec.order[so.entry_of(spec, v)[0]] - 1 - so.entry_of(spec, v)[1], 0) for v in t.ent)
            G = np.float64(t.w) * angle(t, dt)
            while G.shape[-1] - 1 < D:
                G = eo.elevate(G)
            lam = G if lam is None else lam + G
        if lam is not None:
            polys.append(0.0 + lam)
        W = 0.0
        for t in form:
            W += abs(float(t.w))
        out.append((([(t.kind, float(t.w)) for t in trig], lam is not None, W), np.stack(polys, axis=2)))
    return out


def enclose(meta, B):
    """rule 2 on one piece B [np, D + 1]: (plo, phi); a NaN stays"""
    trig, haslin, W = meta
    P = np.zeros(B.shape[1])
    rem = 0.0
    for s, (kind, w) in enumerate(trig):
        th = B[s]
        if np.isnan(th).any():
            return nan, nan
        lo, hi = float(th.min()), float(th.max())
        c = 0.5 * (lo + hi)
        rho = max(hi - c, c - lo)
        S, C = np.sin(c), np.cos(c)
        P = P + (w * (S + C * (th - c)) if kind == SIN else w * (C - S * (th - c)))
        rem = rem + abs(w) * rho * rho * 0.5
    if haslin:
        P = P + B[len(trig)]
    if np.isnan(P).any():
        return nan, nan
    plo, phi = float(P.min()) - rem, float(P.max()) + rem
    if not haslin:
        plo, phi = max(plo, -W), min(phi, W)
    return plo, phi


def end_value(meta, B, last):
    trig, haslin, _ = meta
    v = 0.0
    for s, (kind, w) in enumerate(trig):
        th = B[s][-1 if last else 0]
        v = v + w * float(np.sin(th) if kind == SIN else np.cos(th))
    if haslin:
        v = v + float(B[len(trig)][-1 if last else 0])
    return v


def levels(meta, polys, kn, tol, max_depth=MAX_DEPTH, sides=3, cap=CAP):
    """one form of one problem: polys [l, np, D + 1], kn [l + 1].  bisect_oracle.levels on pieces of several polygons.  Returns ext, when,
    status, npieces and for the tests depth, max_open and margin (the smallest distance of a compared plo / phi from its limit)"""
    kind = (lambda B: [(end_value(meta, B, last), 0, inf) for last in (False, True)], lambda B: enclose(meta, B), bo.halve)
    return bo.levels(kind, [np.array(P, dtype=np.float64) for P in polys], kn, tol, max_depth, sides, cap)


def slack(spec, x, forms, fprm=None, knots=None):
    """[nb, nform]: the header's figure"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb = x.shape[0]
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])

    def S(v):
        o, r = so.entry_of(spec, v)
        hmin = np.diff(np.asarray(spec.knots[o], dtype=np.float64)).min() if knots is None else np.diff(np.asarray(knots), axis=1).min(axis=1)
        return np.abs(x[:, off[o]:off[o + 1]]).max(axis=1) * (2.0 * (spec.order[o] - 1) / hmin) ** r

    out = np.zeros((nb, len(forms)))
    for f, form in enumerate(forms):
        for t in form:
            A = abs(t.phase) + np.abs(_param(t, fprm, nb))
            for v, c in zip(t.ent, t.coef):
                A = A + abs(c) * S(v)
            out[:, f] += 2.0 ** -39 * abs(t.w) * (1.0 + A) + np.where(A > 2.0 ** 11, 2.0 ** -51 * abs(t.w) * A * A, 0.0)
    return out


def values(spec, z, forms, fprm=None):
    """the forms from flag values z [nb, nt, nz] in double precision: [nb, nt, nform]"""
    z = np.asarray(z, dtype=np.float64)
    out = np.zeros(z.shape[:2] + (len(forms),))
    for f, form in enumerate(forms):
        for t in form:
            th = sum(c * z[:, :, v] for v, c in zip(t.ent, t.coef)) + (t.phase + _param(t, fprm, z.shape[0]))[:, None]
            out[:, :, f] += t.w * (np.sin(th) if t.kind == SIN else np.cos(th) if t.kind == COS else th)
    return out


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
    expect: int = OK        # the status every form ends with at TOL
    sl: np.ndarray = None   # slack [nb, nform]
    p0: list = None         # pieces0
    _levels: dict = dataclasses.field(default_factory=dict)

    def kn(self, b, f):
        return self.spec.knots[shape(self.spec, self.forms[f])[0]] if self.knots is None else self.knots[b]

    def levels(self, tol, max_depth=MAX_DEPTH, sides=3):
        """levels of every (problem, form): [nb][nform] dicts (computed once per setting and kept)"""
        key = (tol, max_depth, sides)
        if key not in self._levels:
            self._levels[key] = [[levels(self.p0[f][0], self.p0[f][1][b], self.kn(b, f), tol, max_depth, sides) for f in range(len(self.forms))]
                                 for b in range(self.x.shape[0])]
        return self._levels[key]


TOL = 1e-6     # the tolerance at which the device's decisions are compared with the oracle's
TOL9 = 1e-9    # ... and the one at which only the figures are


def arm_spec(order=6, mult=3, ninterv=4, narms=1, T=5.0):
    return cf.config_E(ninterv=ninterv, order=order, mult=mult, narms=narms, T=T)


def arm_x(spec, nb, seed, amp=0.25):
    """swings of manipulator_bounds' kind: every joint goes linearly from its start to its end angle, perturbed"""
    rng = np.random.default_rng(seed)
    lo, _ = cf.manipulator_bounds(nb, narms=spec.nout // 3, seed=seed)
    nc = spec.ncoef[0]
    f = np.linspace(0.0, 1.0, nc)
    x = np.zeros((nb, spec.nC))
    for o in range(spec.nout):
        a, e = lo[:, 3 * o], lo[:, 3 * spec.nout + 3 * o]
        x[:, o * nc:(o + 1) * nc] = a[:, None] + (e - a)[:, None] * f[None, :] + amp * rng.standard_normal((nb, nc))
    return x


def module_spec(family=0):
    """the plan of the in-tree unicycle module (ntg_amd/modules/unicycle.hip); `family` is the id ntg_family_load gave it"""
    return cf.config_U(family)


# Seeds chosen on the CPU so that every decision of the float64 oracle at TOL keeps 16 slacks from its limit: tests/test_trig_oracle.py
SEEDS = {"TA4": 101, "TE8": 100, "TK8": 100, "TD": 100, "L80": 100, "TPP": 100, "TMOD": 100, "TFULL": 18, "TNAN": 19}
CASES = ["TA4", "TE8", "TK8", "TD", "L80", "TPP", "TMOD"]
_inputs = {}


def inputs(name, family=0):
    if name in _inputs:
        return _inputs[name]
    seed = SEEDS[name]
    if name in ("TA4", "TPP", "TNAN"):
        spec = arm_spec()
        nb = {"TA4": 12, "TPP": 6, "TNAN": 3}[name]
        forms = [tg.tip_height(spec, 0), tg.tip_x(spec, 0), tg.wall(spec, 0, 0.6, 0.8)]
        c = Inputs(name, spec, arm_x(spec, nb, seed), forms)
        if name == "TA4":
            c.forms = forms + [tg.wall(spec, 0, 1.0, 0.5, param=0)]
            c.fprm = np.random.default_rng(seed + 1000).uniform(-0.5, 0.5, (nb, 1))
        if name == "TPP":
            c.knots, c.bps = scaled_grids(spec, np.linspace(0.5, 2.0, nb))
        if name == "TNAN":
            c.x[1, 3] = np.nan
            c.expect = NAN
    elif name == "TE8":
        spec = arm_spec(ninterv=8, narms=2)
        c = Inputs(name, spec, arm_x(spec, 8, seed), [tg.tip_height(spec, 0), tg.tip_x(spec, 0), tg.tip_height(spec, 1), tg.tip_x(spec, 1)])
    elif name == "TK8":
        spec = arm_spec(order=8, mult=4, ninterv=8)   # order 8: the KM = 10 instances
        c = Inputs(name, spec, arm_x(spec, 6, seed), [tg.tip_height(spec, 0), tg.tip_x(spec, 0)])
    elif name == "TD":
        spec = arm_spec()
        e = lambda o, r: tg.entry(spec, o, r)
        # sin(q) + 0.5 cos(q') + 0.25 q'': entries of degrees 5, 4 and 3 in one form, all three kinds
        c = Inputs(name, spec, arm_x(spec, 5, seed), [tg.term(SIN, [e(0, 0)]) + tg.term(COS, [e(1, 1)], w=0.5) + tg.term(LIN, [e(2, 2)], w=0.25),
                                                      tg.term(LIN, [e(0, 0)], w=2.0) + tg.term(LIN, [e(1, 1)], w=-0.5)])
    elif name == "L80":
        spec, x = full_list_problem()   # 80 knot intervals: two level-0 passes
        y = tg.entry(spec, 1, 0)
        c = Inputs(name, spec, np.repeat(x, 2, axis=0), [tg.term(SIN, [y], [0.3]), tg.term(LIN, [y])], expect=FULL)   # all 80 intervals open at level 0
        c.x[1, spec.ncoef[0]:] *= 0.5
    elif name == "TFULL":
        spec = arm_spec()
        c = Inputs(name, spec, arm_x(spec, 2, seed), [tg.term(SIN, [tg.entry(spec, 0, 0)], [40.0])], expect=FULL)
    else:
        spec = module_spec(family)
        e = lambda o, r: tg.entry(spec, o, r)
        c = Inputs(name, spec, np.random.default_rng(seed).standard_normal((8, spec.nC)),
                   [tg.term(SIN, [e(0, 0), e(1, 0)], [1.0, -0.5], phase=0.3) + tg.term(COS, [e(1, 0)]), tg.heading(spec, 1) + tg.heading(spec, 0, kind=SIN, w=0.5)])
    c.sl = slack(spec, np.nan_to_num(c.x), c.forms, c.fprm, c.knots)
    c.p0 = pieces0(spec, c.x, c.forms, c.fprm, c.knots)
    _inputs[name] = c
    return c


def lin_pin_forms(spec):
    """(trig forms, the equivalent ntg_batch_forms forms): all LIN, nent = 1, coef = 1.0, phase = 0, pp = -1 -- rule 5"""
    from ntg_amd import forms as fm
    e = lambda o, r: tg.entry(spec, o, r)
    pairs = [[(e(0, 0), 1.5)], [(e(0, 0), 2.0), (e(1, 1), -0.5)], [(e(2, 2), 0.25), (e(1, 0), 1.0), (e(0, 1), -3.0)]]
    return ([sum((tg.term(LIN, [u], w=w) for u, w in p), []) for p in pairs], [sum((fm.linear(u, w) for u, w in p), []) for p in pairs])


def cross_class_form(spec):
    """config_T's refusal: a form across its two basis classes"""
    return tg.term(SIN, [tg.entry(spec, 0, 0), tg.entry(spec, 2, 0)])
