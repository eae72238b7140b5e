"""Constructors for the min / max expressions Plan.minmax (ntg_batch_minmax) certifies: polygons, boxes, corridors, unions of discs.

A declaration is a pair (forms, group): forms as Plan.forms takes them (ntg_amd.forms), and a group (outer, inner, clauses) whose clauses are
lists of members (form, c, pc) -- the function q_form(z) + c + fprm[pc] -- with form an index into that list of forms:

    from ntg_amd import minmax as mm
    square = mm.polygon(spec, 0, 1, [(18, -1), (22, -1), (22, 2), (18, 2)])     # > 0 outside, < 0 inside
    lane = mm.corridor(spec, 0, 1, [(5, 0, 6, 2), (12, 1, 4, 2, 0.3)])           # <= 0 inside one box at least
    forms, groups = mm.merge(square, lane)
    out = plan.minmax(x, forms, groups, tol=1e-6)
    outside = out["ext"][:, 0, 0] >= 0      # min over t of max over faces: the square is never entered
    inside = out["ext"][:, 1, 3] <= 0       # max over t of min over boxes of max over faces: the corridor is never left

Every face is the signed distance n . (p - v) to the line through a vertex v with the OUTWARD unit normal n, so a polygon's group is negative
inside, positive outside, and its value outside is a lower bound of the distance to the polygon.  include/ntg_amd.h has the definition.
"""
from __future__ import annotations

import math
from typing import Sequence

from . import forms as fm

MIN, MAX = 0, 1            # NTG_MINMAX_MIN, NTG_MINMAX_MAX
MAXFORMS = 16              # NTG_MINMAX_MAXFORMS
MAXTERMS = 40              # NTG_MINMAX_MAXTERMS, all forms together
MAXGROUPS = 4              # NTG_MINMAX_MAXGROUPS
MAXCLAUSES = 8             # NTG_MINMAX_MAXCLAUSES, per group
MAXMEMBERS = 16            # NTG_MINMAX_MAXMEMBERS, per group


def halfplane(spec, ox: int, oy: int, nx: float, ny: float, px: float, py: float, pcx: int = -1, pcy: int = -1) -> list:
    """the form nx (x - px - fprm[pcx]) + ny (y - py - fprm[pcy]) of outputs ox, oy: the signed distance, for a unit normal, to the line
    through (px, py) (+ the centre in fprm), positive on the side the normal points to"""
    return fm.linear(fm.entry(spec, ox, 0), nx, px, pcx) + fm.linear(fm.entry(spec, oy, 0), ny, py, pcy)


def polygon(spec, ox: int, oy: int, vertices: Sequence, centre_params=None) -> tuple:
    """(forms, group) of a convex polygon with counter-clockwise vertices [(x, y), ...]: one form per edge, the signed distance to the edge's
    line with the outward normal, and the group MAX over them -- negative inside, positive outside.  centre_params = (pcx, pcy): the vertices
    are relative to the centre (fprm[pcx], fprm[pcy]) of every problem.  Raises ValueError for fewer than 3 vertices, a clockwise or a
    non-convex polygon, or a repeated vertex."""
    v = [(float(x), float(y)) for x, y in vertices]
    n = len(v)
    if n < 3:
        raise ValueError("a polygon needs 3 vertices at least")
    if n > MAXMEMBERS:
        raise ValueError(f"a polygon takes up to {MAXMEMBERS} vertices")
    pcx, pcy = (-1, -1) if centre_params is None else centre_params
    edges = [(v[(i + 1) % n][0] - v[i][0], v[(i + 1) % n][1] - v[i][1]) for i in range(n)]
    for i in range(n):
        (ax, ay), (bx, by) = edges[i], edges[(i + 1) % n]
        if math.hypot(ax, ay) == 0.0:
            raise ValueError(f"vertex {i} is repeated")
        if not ax * by - ay * bx > 0.0:
            raise ValueError(f"the polygon is not convex and counter-clockwise at vertex {(i + 1) % n}")
    forms = []
    for (x, y), (ex, ey) in zip(v, edges):
        ln = math.hypot(ex, ey)
        forms.append(halfplane(spec, ox, oy, ey / ln, -ex / ln, x, y, pcx, pcy))
    return forms, (MIN, MAX, [[(f, 0.0, -1) for f in range(n)]])


def _corners(cx, cy, hx, hy, angle=0.0):
    c, s = math.cos(angle), math.sin(angle)
    return [(cx + c * a - s * b, cy + s * a + c * b) for a, b in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def box(spec, ox: int, oy: int, cx: float, cy: float, hx: float, hy: float, angle: float = 0.0, centre_params=None) -> tuple:
    """(forms, group) of the box with centre (cx, cy), half sides hx, hy, turned by angle: polygon() of its four corners"""
    if not (hx > 0.0 and hy > 0.0):
        raise ValueError("the half sides of a box must be positive")
    return polygon(spec, ox, oy, _corners(cx, cy, hx, hy, angle), centre_params)


def corridor(spec, ox: int, oy: int, boxes: Sequence) -> tuple:
    """(forms, group) of a corridor of overlapping boxes [(cx, cy, hx, hy[, angle]), ...]: MIN over the boxes of MAX over each box's faces,
    <= 0 where the point is inside one box at least.  max over t <= 0 certifies that the corridor is never left."""
    if not 1 <= len(boxes) <= MAXCLAUSES:
        raise ValueError(f"a corridor takes 1 .. {MAXCLAUSES} boxes")
    forms, clauses = [], []
    for b in boxes:
        f, (_, _, cl) = box(spec, ox, oy, *b)
        clauses.append([(len(forms) + m, c, pc) for m, c, pc in cl[0]])
        forms += f
    if len(forms) > MAXMEMBERS:
        raise ValueError(f"a group takes up to {MAXMEMBERS} members")
    return forms, (MIN, MAX, clauses)


def discs(spec, ox: int, oy: int, discs: Sequence) -> tuple:
    """(forms, group) of a union of discs [(cx, cy, r[, pcx, pcy]), ...]: MIN over the discs of d^2 - r^2 with d the distance to the centre
    (cx + fprm[pcx], cy + fprm[pcy]) -- <= 0 where the point is within range of one at least (coverage: max over t <= 0), >= 0 where it is
    outside all of them (obstacles: min over t >= 0)."""
    if not 1 <= len(discs) <= MAXMEMBERS:
        raise ValueError(f"a group takes 1 .. {MAXMEMBERS} members")
    forms, members = [], []
    for d in discs:
        cx, cy, r = (float(a) for a in d[:3])
        pcx, pcy = (int(d[3]), int(d[4])) if len(d) > 3 else (-1, -1)
        members.append((len(forms), -(r * r), -1))
        forms.append(fm.square(fm.entry(spec, ox, 0), cx, pcx) + fm.square(fm.entry(spec, oy, 0), cy, pcy))
    return forms, (MIN, MIN, [members])


def merge(*parts) -> tuple:
    """(forms, groups) of several (forms, group) declarations for one call: the forms concatenated, a form that several parts declare with
    the same terms kept once, every group's form indices renumbered"""
    forms, groups = [], []
    for f, (outer, inner, clauses) in parts:
        at = []
        for form in f:
            form = list(form)
            if form not in forms:
                forms.append(form)
            at.append(forms.index(form))
        groups.append((outer, inner, [[(at[m], c, pc) for m, c, pc in cl] for cl in clauses]))
    if len(forms) > MAXFORMS or len(groups) > MAXGROUPS or sum(len(f) for f in forms) > MAXTERMS:
        raise ValueError(f"one call takes up to {MAXFORMS} forms of {MAXTERMS} terms together and {MAXGROUPS} groups")
    return forms, groups
