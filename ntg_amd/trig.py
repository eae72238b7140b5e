"""Constructors for the sums of sines and cosines Plan.trig (ntg_batch_trig) certifies, so that nobody writes flag indices by hand.

A form is a list of Term; the constructors return such lists, and `+` concatenates them:

    from ntg_amd import trig as tg
    height = tg.tip_height(spec, 0)                        # sin qa + sin(qa + qb) + sin(qa + qb + qc) of arm 0
    reach = tg.tip_x(spec, 0)                              # the same with cosines
    out = plan.trig(x, [height, reach], tol=1e-9, lower=lo, upper=up)

A term is w g(theta) with theta = sum_i coef[i] z[ent[i]] + phase + fprm[pp] (a parameter index of -1 reads none) and g = sin, cos or the
identity by kind: include/ntg_amd.h has the definition.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

from .forms import entry

MAXFORMS = 8   # NTG_TRIG_MAXFORMS
MAXTERMS = 4   # NTG_TRIG_MAXTERMS, per form
MAXENT = 4     # NTG_TRIG_MAXENT, flag entries per angle
SIN, COS, LIN = 0, 1, 2


class Term(NamedTuple):
    kind: int
    ent: tuple
    coef: tuple
    phase: float
    pp: int
    w: float


def term(kind: int, ents: Sequence[int], coefs: Sequence[float] = None, phase: float = 0.0, param: int = -1, w: float = 1.0) -> list:
    """w g(sum_i coefs[i] z[ents[i]] + phase + fprm[param]); coefs default to ones"""
    ents = tuple(int(e) for e in ents)
    coefs = tuple(1.0 for _ in ents) if coefs is None else tuple(float(c) for c in coefs)
    if not 1 <= len(ents) <= MAXENT or len(coefs) != len(ents):
        raise ValueError(f"an angle takes 1 .. {MAXENT} flag entries, with one coefficient each")
    if kind not in (SIN, COS, LIN):
        raise ValueError("kind is one of SIN, COS, LIN")
    return [Term(int(kind), ents, coefs, float(phase), int(param), float(w))]


def sin_sum(spec, outputs: Sequence[int], kind: int = SIN, phase: float = 0.0, param: int = -1, w: float = 1.0, deriv: int = 0) -> list:
    """sum over n of w g(z_{o_1} + .. + z_{o_n} + phase + fprm[param]): the partial sums of the outputs' angles, as the links of a planar
    arm add up (g = sin by default)"""
    outputs = list(outputs)
    if not 1 <= len(outputs) <= min(MAXTERMS, MAXENT):
        raise ValueError(f"1 .. {min(MAXTERMS, MAXENT)} outputs")
    return [t for n in range(1, len(outputs) + 1) for t in term(kind, [entry(spec, o, deriv) for o in outputs[:n]], None, phase, param, w)]


def _arm(spec, arm: int):
    if not 0 <= 3 * arm + 2 < spec.nout:
        raise ValueError(f"arm {arm}: the spec has {spec.nout // 3} arms of three joints")
    return [3 * arm, 3 * arm + 1, 3 * arm + 2]


def tip_height(spec, arm: int) -> list:
    """sin qa + sin(qa + qb) + sin(qa + qb + qc) of planar 3-link arm `arm` (outputs 3 arm .. 3 arm + 2): the manipulator family's row"""
    return sin_sum(spec, _arm(spec, arm))


def tip_x(spec, arm: int) -> list:
    """cos qa + cos(qa + qb) + cos(qa + qb + qc): the tip's x-coordinate"""
    return sin_sum(spec, _arm(spec, arm), kind=COS)


def wall(spec, arm: int, nx: float, ny: float, param: int = -1) -> list:
    """n . tip = |n| (sin(qa + phi) + sin(qa + qb + phi) + sin(qa + qb + qc + phi)) with phi = atan2(nx, ny): the tip stays behind the wall
    n . p <= d where this form is <= d.  param: a per-problem rotation of the wall added to phi"""
    return sin_sum(spec, _arm(spec, arm), phase=math.atan2(nx, ny), param=param, w=math.hypot(nx, ny))


def heading(spec, output: int, kind: int = LIN, w: float = 1.0, deriv: int = 0) -> list:
    """w g(z_output): a heading-angle output itself (LIN), or its sine or cosine"""
    return term(kind, [entry(spec, output, deriv)], w=w)
