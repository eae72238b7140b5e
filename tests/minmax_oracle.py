"""ntg_batch_minmax's definition (include/ntg_amd.h) for the tests, decision by decision in float64, and the inputs the CPU and GPU tests share.

  pieces0   level-0 pieces of every group: forms_oracle.form_polygons of the members' forms, + d on every point (a member with pc = -1 and
            c = 0.0 adds nothing), elevated to the group's degree (rule 1).
  lattice   OUTER_k INNER_j of one figure per member, with the member that decides it (ties: smallest index, smallest clause) and `gap`,
            the smallest difference that, reversed, would name another member.
  levels    the level loop of ntg_batch_extrema (bisect_oracle.levels) on those pieces with the enclosure of rule 2 and the ends of rule 3.
            It records the depth, the most pieces open at a level, `margin` (the smallest distance of any open / retire decision from its
            limit) and `tie` (the lattice gap at the two ends that are returned).
  slack     max over the members of 2^-39 (M_f + |d|), M_f forms_oracle's sum.
  values    the groups from flag values, for the sampled extrema.

A group is (outer, inner, clauses), a clause a list of members (form, c, pc): ntg_amd.minmax.  Shapes are small: each case is the smallest at
which its path can still go wrong.
"""
import dataclasses
import math
from math import inf, nan

import numpy as np

import bisect_oracle as bo
import envelope_oracle as eo
import forms_oracle as fo
from bisect_oracle import CAP, DEPTH, FULL, MAX_DEPTH, NAN, OK, violation   # (the tests take them from here)
from cert_common import full_list_problem, greville, scaled_grids
from ntg_amd import configs as cf, forms as fm, minmax as mm

MIN, MAX = mm.MIN, mm.MAX


def members(group):
    """the group's concatenated member list and, per member, its clause"""
    flat = [m for cl in group[2] for m in cl]
    return flat, [k for k, cl in enumerate(group[2]) for _ in cl]


def shape(spec, forms, group):
    """(output whose knot intervals the group has, degree D of its polygons); raises if the group names two basis classes"""
    sh = [fo.shape(spec, forms[f]) for f, _, _ in members(group)[0]]
    assert all(fo.so.same_class(spec, o, sh[0][0]) for o, _ in sh), "the group names forms of different basis classes"
    return sh[0][0], max(D for _, D in sh)


def offsets(group, fprm, nb):
    """d [nb, nm] = c + fprm[pc], one rounding"""
    return np.stack([np.float64(c) + (np.asarray(fprm, dtype=np.float64)[:, pc] if pc >= 0 else np.zeros(nb)) for _, c, pc in members(group)[0]], axis=1)


def pieces0(spec, x, forms, groups, fprm=None, knots=None):
    """per group P [nb, l, nm, D + 1]"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nb = x.shape[0]
    polys = fo.form_polygons(spec, x, forms, fprm, knots)
    out = []
    for g in groups:
        _, D = shape(spec, forms, g)
        d = offsets(g, fprm, nb)
        per = []
        for m, (f, c, pc) in enumerate(members(g)[0]):
            G = polys[f]
            if pc >= 0 or c != 0.0:
                G = G + d[:, m][:, None, None]
            while G.shape[-1] - 1 < D:
                G = eo.elevate(G)
            per.append(G)
        out.append(np.stack(per, axis=2))
    return out


def lattice(group, vals):
    """(OUTER_k INNER_j vals, the member that decides it, gap); vals [nm].  gap: the smallest |difference| between the deciding member's value
    and another member's of its clause, or between the deciding clause's value and another clause's"""
    outer, inner, clauses = group
    pick = lambda mx, a, b: (a > b) if mx else (a < b)
    m, best, gap = 0, None, inf
    per = []
    for cl in clauses:
        cv, cw = None, -1
        for _ in cl:
            v = float(vals[m])
            if cv is None or pick(inner == MAX, v, cv):
                cv, cw = v, m
            m += 1
        per.append((cv, cw, m - len(cl), m))
    for cv, cw, a, b in per:
        if best is None or pick(outer == MAX, cv, best[0]):
            best = (cv, cw, a, b)
    for cv, cw, a, b in per:
        if cw != best[1]:
            gap = min(gap, abs(cv - best[0]))
    for j in range(best[2], best[3]):
        if j != best[1]:
            gap = min(gap, abs(float(vals[j]) - best[0]))
    return best[0], best[1], gap


def enclose(group, B):
    """rule 2 on one piece B [nm, D + 1]: (plo, phi); a NaN in any member's figures gives NaN"""
    if np.isnan(B).any():
        return nan, nan
    return lattice(group, B.min(axis=1))[0], lattice(group, B.max(axis=1))[0]


def levels(group, polys, kn, tol, max_depth=MAX_DEPTH, sides=3, cap=CAP):
    """one group of one problem: polys [l, nm, D + 1], kn [l + 1].  bisect_oracle.levels on pieces of several polygons: the deciding member
    breaks the ties of the ends and its lattice gap is carried along.  Returns ext, when, which, status, npieces and for the tests depth,
    max_open, margin and tie"""
    kind = (lambda B: [lattice(group, B[:, col]) for col in (0, -1)], lambda B: enclose(group, B), bo.halve)
    return bo.levels(kind, [np.array(P, dtype=np.float64) for P in polys], kn, tol, max_depth, sides, cap)


def slack(spec, x, forms, groups, fprm=None, knots=None):
    """[nb, ngroup]: the header's figure"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    Mf = fo.slack(spec, x, forms, fprm, knots)   # 2^-39 M_f
    out = np.zeros((x.shape[0], len(groups)))
    for g, grp in enumerate(groups):
        d = offsets(grp, fprm, x.shape[0])
        for m, (f, _, _) in enumerate(members(grp)[0]):
            out[:, g] = np.maximum(out[:, g], Mf[:, f] + 2.0 ** -39 * np.abs(d[:, m]))
    return out


def member_values(spec, z, forms, group, fprm=None):
    """the group's members from flag values z [nb, nt, nz]: [nb, nt, nm]"""
    q = fo.values(spec, z, forms, fprm)
    d = offsets(group, fprm, q.shape[0])
    return np.stack([q[:, :, f] + d[:, m][:, None] for m, (f, _, _) in enumerate(members(group)[0])], axis=2)


def fold(group, mv):
    """OUTER_k INNER_j over the last axis of mv [..., nm]"""
    outer, inner, clauses = group
    red = lambda mx: np.max if mx else np.min
    at, per = 0, []
    for cl in clauses:
        per.append(red(inner == MAX)(mv[..., at:at + len(cl)], axis=-1))
        at += len(cl)
    return red(outer == MAX)(np.stack(per, axis=-1), axis=-1)


def values(spec, z, forms, groups, fprm=None):
    """the groups from flag values z [nb, nt, nz] in double precision: [nb, nt, ngroup]"""
    return np.stack([fold(g, member_values(spec, z, forms, g, fprm)) for g in groups], axis=2)


def negated(forms, groups, fprm):
    """the declaration of -h: every w and every c negated, MIN and MAX swapped, and the fprm columns that members name through pc negated
    (no form of the tests reads those columns as a shift)"""
    nf = [[t._replace(w=-t.w) for t in f] for f in forms]
    ng = [(1 - o, 1 - i, [[(f, -c, pc) for f, c, pc in cl] for cl in cls]) for o, i, cls in groups]
    if fprm is not None:
        fprm = np.array(fprm, dtype=np.float64)
        cols = sorted({pc for g in groups for _, _, pc in members(g)[0] if pc >= 0})
        assert not any(p in cols for f in forms for t in f for p in (t.pu, t.pv))
        fprm[:, cols] = -fprm[:, cols]
    return nf, ng, fprm


# ---------------- the inputs of the tests ----------------
@dataclasses.dataclass
class Inputs:
    name: str
    spec: object
    x: np.ndarray
    forms: list
    groups: list
    fprm: object = None
    knots: object = None    # [nb, l + 1]: per-problem grids
    bps: object = None
    expect: int = OK        # the status every group ends with at TOL
    sl: np.ndarray = None   # slack [nb, ngroup]
    p0: list = None         # pieces0
    _levels: dict = dataclasses.field(default_factory=dict)

    def kn(self, b, g):
        return self.spec.knots[shape(self.spec, self.forms, self.groups[g])[0]] if self.knots is None else self.knots[b]

    def levels(self, tol, max_depth=MAX_DEPTH, sides=3):
        """levels of every (problem, group): [nb][ngroup] dicts (computed once per setting and kept)"""
        key = (tol, max_depth, sides)
        if key not in self._levels:
            self._levels[key] = [[levels(self.groups[g], self.p0[g][b], self.kn(b, g), tol, max_depth, sides) for g in range(len(self.groups))]
                                 for b in range(self.x.shape[0])]
        return self._levels[key]


TOL = 1e-6     # the tolerance at which the device's decisions are compared with the oracle's
TOL9 = 1e-9    # ... and the one at which only the figures are


def kincar_spec(order=6, mult=3, l=4):
    return cf._kincar_spec(1, order, mult, l, 5 * l + 1, 5.0, f"kincar-2out-k{order}-l{l}")


def ngon(n, cx, cy, r, phase=0.1):
    return [(cx + r * math.cos(phase + 2.0 * math.pi * i / n), cy + r * math.sin(phase + 2.0 * math.pi * i / n)) for i in range(n)]


def module_spec(family=0):
    """the plan of the in-tree unicycle module (ntg_amd/modules/unicycle.hip); `family` is the id ntg_family_load gave it"""
    return cf.config_U(family)


# Seeds chosen on the CPU so that every decision of the float64 oracle at TOL keeps 16 slacks from its limit: tests/test_minmax_oracle.py
SEEDS = {"MS20": 100, "MP4": 101, "MQ8": 100, "MK8": 101, "M16": 100, "MPP": 106, "MMOD": 100, "ML80": 100, "MFULL": 100, "MNAN": 100}
CASES = ["MP4", "MQ8", "MK8", "M16", "MS20", "MPP", "MMOD", "ML80"]
CASES9 = ["M16", "MS20"]      # the cases whose kinks close to 1e-9 within depth 30: h * slope below 1 (the others end in DEPTH there)
_inputs = {}


def mp4_declaration(spec):
    """four groups in one call: a triangle around the per-problem centre fprm[0:2], a box, a corridor of two boxes whose first is that box
    (merge keeps its forms once), and MIN of two discs with c = -r^2, the second one's through fprm[2]"""
    tri = mm.polygon(spec, 0, 1, [(-2.0, -1.5), (2.0, -1.5), (0.0, 2.0)], centre_params=(0, 1))
    boxes = [(10.0, 0.5, 12.0, 4.0), (30.0, 0.0, 12.0, 5.0, 0.05)]
    dforms, (o, i, (cl,)) = mm.discs(spec, 0, 1, [(15.0, 0.5, 2.0), (28.0, 0.0, 3.0)])
    return mm.merge(tri, mm.box(spec, 0, 1, *boxes[0]), mm.corridor(spec, 0, 1, boxes), (dforms, (o, i, [[cl[0], (cl[1][0], 0.0, 2)]])))


def inputs(name, family=0):
    if name in _inputs:
        return _inputs[name]
    seed = SEEDS[name]
    rng = np.random.default_rng(seed + 1000)
    if name in ("MP4", "MNAN"):
        spec = kincar_spec()
        nb = 12 if name == "MP4" else 3
        forms, groups = mp4_declaration(spec)
        c = Inputs(name, spec, fo.kincar_x(spec, nb, seed), forms, groups, fprm=np.stack([rng.uniform(10.0, 30.0, nb), rng.uniform(-1.0, 1.0, nb), -rng.uniform(4.0, 9.0, nb)], axis=1))
        if name == "MNAN":
            c.x[1, 3] = np.nan
            c.expect = NAN
    elif name == "MQ8":
        spec = kincar_spec(l=8)
        disc, (_, _, cl) = mm.discs(spec, 0, 1, [(20.0, 0.5, 3.0)])
        c = Inputs(name, spec, fo.kincar_x(spec, 8, seed), disc + [mm.halfplane(spec, 0, 1, 0.6, 0.8, 22.0, 1.0)], [(MAX, MAX, [cl[0] + [(1, 0.0, -1)]])])   # degrees 10 and 5
    elif name == "MK8":
        spec = kincar_spec(order=8, mult=4, l=4)   # order 8: the 19-point instance
        forms, groups = mm.merge(mm.box(spec, 0, 1, 20.0, 0.5, 3.0, 2.0, 0.3), mm.discs(spec, 0, 1, [(12.0, 0.0, 2.0), (30.0, 1.0, 2.5)]))
        c = Inputs(name, spec, fo.kincar_x(spec, 6, seed), forms, groups)
    elif name == "MS20":
        # slow cars on short intervals, h * slope about 0.5: the kinks of a polygon close to 1e-9 within depth 30 (about log2(h * slope / tol) levels)
        spec = kincar_spec(l=20)
        gv = greville(spec)
        g2 = np.random.default_rng(seed)
        x = np.concatenate([gv[None, :] + 0.05 * g2.standard_normal((6, gv.size)), 0.2 + 0.15 * g2.standard_normal((6, gv.size))], axis=1)
        forms, groups = mm.merge(mm.polygon(spec, 0, 1, [(2.0, -0.2), (3.0, -0.1), (2.4, 0.6)]), mm.box(spec, 0, 1, 4.0, 0.2, 0.5, 0.3, 0.2))
        c = Inputs(name, spec, x, forms, groups)
    elif name == "M16":
        spec = kincar_spec()
        forms, group = mm.polygon(spec, 0, 1, ngon(16, 20.0, 0.5, 3.0))   # 16 members: half the wavefronts
        c = Inputs(name, spec, fo.kincar_x(spec, 6, seed), forms, [group])
    elif name == "MPP":
        spec = kincar_spec()
        nb = 6
        forms, groups = mm.merge(mm.box(spec, 0, 1, 20.0, 0.5, 3.0, 2.0, 0.3), mm.discs(spec, 0, 1, [(12.0, 0.0, 2.0), (30.0, 1.0, 2.5)]))
        c = Inputs(name, spec, fo.kincar_x(spec, nb, seed), forms, groups)
        scales = np.linspace(0.5, 2.0, nb)
        c.knots, c.bps = scaled_grids(spec, scales)
    elif name in ("ML80", "MFULL"):
        spec, x = full_list_problem()   # 80 knot intervals: two level-0 passes
        if name == "ML80":   # the route's x is monotone: the half planes across it close within a few levels
            forms, groups = mm.merge(mm.box(spec, 0, 1, 20.0, 0.0, 3.0, 5.0, 0.2))
            c = Inputs(name, spec, np.repeat(x, 2, axis=0), forms, groups)
        else:                # y repeats one shape on every interval: all 80 are open at level 0
            y = fm.entry(spec, 1, 0)
            c = Inputs(name, spec, np.repeat(x, 2, axis=0), [fm.linear(y, 1.0), fm.linear(y, -0.5)], [(MAX, MAX, [[(0, 0.0, -1), (1, 0.25, -1)]])], expect=FULL)
        c.x[1, spec.ncoef[0]:] *= 0.5
    else:
        spec = module_spec(family)
        forms, groups = mm.merge(mm.polygon(spec, 0, 1, ngon(5, 0.2, -0.1, 0.8)), mm.discs(spec, 0, 1, [(0.5, 0.5, 0.6), (-0.6, 0.0, 0.5)]))
        c = Inputs(name, spec, np.random.default_rng(seed).standard_normal((8, spec.nC)), forms, groups)
    c.sl = slack(spec, np.nan_to_num(c.x), c.forms, c.groups, c.fprm, c.knots)
    c.p0 = pieces0(spec, c.x, c.forms, c.groups, c.fprm, c.knots)
    _inputs[name] = c
    return c


def single_member(form=0):
    """pin 1: one clause of one member, c = 0.0, pc = -1"""
    return (MIN, MAX, [[(form, 0.0, -1)]])


def cross_class_declaration(spec):
    """config_T's refusal: a group over forms of its two basis classes"""
    return [fm.linear(fm.entry(spec, 0, 0), 1.0), fm.linear(fm.entry(spec, 2, 0), 1.0)], [(MAX, MAX, [[(0, 0.0, -1), (1, 0.0, -1)]])]
