"""Constructors for the quadratic forms Plan.forms (ntg_batch_forms) certifies, so that nobody writes flag indices by hand.

A form is a list of Term; the constructors return such lists, and `+` concatenates them:

    from ntg_amd import forms as fm
    x1, y1 = fm.entry(spec, 0, 1), fm.entry(spec, 1, 1)
    speed2 = fm.square(x1) + fm.square(y1)                 # == fm.speed2(spec, (0, 1))
    turn = fm.cross(spec, (0, 1), (1, 1))                  # x' y'' - y' x''
    out = plan.forms(x, [speed2, turn], tol=1e-9)

A term is w (z[u] - a)(z[v] - b), or w (z[u] - a) when v == -1, with a = su + fprm[pu] and b = sv + fprm[pv] (a parameter index of -1 reads
none): include/ntg_amd.h has the definition.

Plan.ratios (ntg_batch_ratios) certifies ratios of products of such forms; a ratio is a pair (num, den) of lists of form indices:

    forms, kappa2 = fm.curvature2(spec, (0, 1))            # [speed2, cross], ([1, 1], [0, 0, 0]): T T / (S S S)
    out = plan.ratios(x, forms, [kappa2], tol=1e-9)
    tan_max = fm.steering_tan_max(out, wheelbase=3.0)      # certified max |tan delta| per problem
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

import numpy as np

MAXFORMS = 8   # NTG_FORM_MAXFORMS
MAXTERMS = 8   # NTG_FORM_MAXTERMS, per form
MAXRATIOS = 4     # NTG_RATIO_MAXRATIOS
MAXFACTORS = 4    # NTG_RATIO_MAXFACTORS, per side of a ratio


class Term(NamedTuple):
    u: int
    v: int
    pu: int
    pv: int
    w: float
    su: float
    sv: float


def entry(spec, output: int, deriv: int) -> int:
    """the flag entry iz[output] + deriv of derivative `deriv` of output `output`, in the layout of Plan.interp"""
    if not 0 <= output < spec.nout:
        raise ValueError(f"output {output}: the spec has outputs 0 .. {spec.nout - 1}")
    if not 0 <= deriv < spec.maxderiv[output]:
        raise ValueError(f"derivative {deriv} of output {output}: the flag holds 0 .. {spec.maxderiv[output] - 1}")
    return int(sum(spec.maxderiv[:output])) + int(deriv)


def square(u: int, shift: float = 0.0, param: int = -1, w: float = 1.0) -> list:
    """w (z[u] - shift - fprm[param])^2"""
    return [Term(int(u), int(u), int(param), int(param), float(w), float(shift), float(shift))]


def product(u: int, v: int, w: float = 1.0, su: float = 0.0, sv: float = 0.0, pu: int = -1, pv: int = -1) -> list:
    """w (z[u] - su - fprm[pu]) (z[v] - sv - fprm[pv])"""
    return [Term(int(u), int(v), int(pu), int(pv), float(w), float(su), float(sv))]


def linear(u: int, w: float, shift: float = 0.0, param: int = -1) -> list:
    """w (z[u] - shift - fprm[param])"""
    return [Term(int(u), -1, int(param), -1, float(w), float(shift), 0.0)]


def speed2(spec, outs: Sequence[int]) -> list:
    """sum over the outputs of (z_o')^2: the squared speed of the body whose coordinates they are"""
    return [t for o in outs for t in square(entry(spec, o, 1))]


def cross(spec, x, y) -> list:
    """z_x^(rx) z_y^(ry + 1) - z_y^(ry) z_x^(rx + 1) for x = (ox, rx), y = (oy, ry); with rx = ry = 1 the turning numerator x' y'' - y' x''"""
    (ox, rx), (oy, ry) = x, y
    return product(entry(spec, ox, rx), entry(spec, oy, ry + 1), 1.0) + product(entry(spec, oy, ry), entry(spec, ox, rx + 1), -1.0)


def ellipse(spec, ox: int, oy: int, ax: float, ay: float, pcx: int, pcy: int) -> list:
    """((x - fprm[pcx]) / ax)^2 + ((y - fprm[pcy]) / ay)^2: >= 1 outside the ellipse with half axes ax, ay around the centre in fprm"""
    return square(entry(spec, ox, 0), param=pcx, w=1.0 / (ax * ax)) + square(entry(spec, oy, 0), param=pcy, w=1.0 / (ay * ay))


def steering_bound(ext, wheelbase: float, speed_form: int = 0, cross_form: int = 1) -> np.ndarray:
    """Conservative certificate of the kinematic car's steering over the whole horizon from Plan.forms' ext [batch, nform, 4], where form
    speed_form is speed2 and form cross_form is cross(spec, (ox, 1), (oy, 1)).  With N = max(|min_lo|, |max_hi|) of the cross form and
    m = min_lo of speed2, |kappa| = |x' y'' - y' x''| / v^3 <= N / m^1.5 wherever m > 0, hence |tan delta| <= wheelbase N / m^1.5.
    Returns [batch]; inf where m <= 0 (the flat map is singular at v = 0: no statement)."""
    e = ext.detach().cpu().numpy() if hasattr(ext, "detach") else np.asarray(ext, dtype=np.float64)
    n = np.maximum(np.abs(e[:, cross_form, 0]), np.abs(e[:, cross_form, 3]))
    m = e[:, speed_form, 0]
    out = np.full(e.shape[0], math.inf)
    ok = m > 0.0
    out[ok] = wheelbase * n[ok] / m[ok] ** 1.5
    return out


def ratio(num: Sequence[int], den: Sequence[int] = ()) -> tuple:
    """the product of the forms num over the product of the forms den (indices into the call's list of forms; an empty side is 1, a repeated
    index a power)"""
    num, den = [int(f) for f in num], [int(f) for f in den]
    if not num and not den:
        raise ValueError("a ratio needs a form on one side at least")
    if len(num) > MAXFACTORS or len(den) > MAXFACTORS:
        raise ValueError(f"a side of a ratio takes up to {MAXFACTORS} forms")
    return num, den


def curvature2(spec, outs: Sequence[int]) -> tuple:
    """(forms, ratio) of the squared curvature kappa^2 = T T / (S S S) of the planar body with coordinates outs = (ox, oy): forms =
    [S, T] = [speed2, cross], to be passed first in the call's list of forms (or shift the ratio's indices)"""
    ox, oy = outs
    return [speed2(spec, (ox, oy)), cross(spec, (ox, 1), (oy, 1))], ratio([1, 1], [0, 0, 0])


def lateral_accel2(spec, outs: Sequence[int]) -> tuple:
    """(forms, ratio) of the squared lateral acceleration (v^2 kappa)^2 = T T / S, forms = [S, T] as in curvature2"""
    ox, oy = outs
    return [speed2(spec, (ox, oy)), cross(spec, (ox, 1), (oy, 1))], ratio([1, 1], [0])


def steering_tan_max(out, wheelbase: float, ratio_index: int = 0) -> np.ndarray:
    """Certified largest |tan delta| = wheelbase |kappa| of the kinematic car over the whole horizon, from Plan.ratios' result `out` whose
    ratio ratio_index is curvature2: wheelbase sqrt(max_hi).  Returns [batch]; inf where the status is not OK (a pole of the flat map at
    v = 0, NaN, or a bisection that stopped early: no statement)."""
    get = lambda k: out[k].detach().cpu().numpy() if hasattr(out[k], "detach") else np.asarray(out[k])
    hi, st = get("ext")[:, ratio_index, 3].astype(np.float64), get("status")[:, ratio_index]
    res = np.full(hi.shape[0], math.inf)
    ok = (st == 0) & (hi >= 0.0)
    res[ok] = wheelbase * np.sqrt(hi[ok])
    return res
