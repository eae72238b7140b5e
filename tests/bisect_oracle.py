"""The level loop of ntg_batch_extrema's definition (include/ntg_amd.h), written once in float64 for every bisection call: the one sequence of
end-takings, open / retire decisions and halvings that the device's level loops (ext_levels and its threshold instance, ratio_levels,
trig_levels, minmax_levels) are tested against.  The oracles of the calls hand it their kind of piece and their level-0 pieces:

  extrema_oracle, forms_oracle   a polygon                                  POLYGON
  separation_oracle              a polygon, sides = 1 and the threshold s2  POLYGON
  ratios_oracle                  a numerator / denominator pair
  trig_oracle                    the angle polygons of a form's terms
  minmax_oracle                  the members' polygons of a group

A kind of piece is (ends, enclose, halves), three functions of a piece B:
  ends(B)      its two end values, each (v, w, fig): the value (None: no value there, a pole), the tie-break index of whatever decides it
               and a figure carried along with the end if it is taken.  A kind without either gives 0 and inf.
  enclose(B)   (plo, phi); (nan, nan) where a NaN is involved, (-inf, inf) where there is no bound.
  halves(B)    (left, right) by de Casteljau: halve() below, on every polygon of the piece.

Also here, because every oracle has them alike: the status codes, CAP and MAX_DEPTH, and violation (rule 7)."""
from math import inf, isnan, nan

import numpy as np

from ntg_amd import configs as cf

OK, DEPTH, FULL, NAN, POLE, NONE, BADPAIR = 0, 1, 2, 3, 4, -1, -2
CAP, MAX_DEPTH = 64, 30
INF_BOUND = cf.INF_BOUND


def halve(B):
    """(left, right) of a polygon [D + 1] of floats, or of a stack of polygons [np, D + 1] in numpy rows: every sum is 0.5 * (a + b)"""
    if isinstance(B, np.ndarray):
        R, L = B.copy(), np.empty_like(B)
        L[:, 0] = B[:, 0]
        n = B.shape[1]
        for r in range(1, n):
            R[:, :n - r] = 0.5 * (R[:, :n - r] + R[:, 1:n - r + 1])
            L[:, r] = R[:, 0]
        return L, R
    R, L = list(B), [B[0]]
    for r in range(1, len(B)):
        for s in range(len(B) - r):
            R[s] = 0.5 * (R[s] + R[s + 1])
        L.append(R[0])
    return L, R


def _polygon_hull(B):
    return (nan, nan) if any(isnan(v) for v in B) else (min(B), max(B))


POLYGON = (lambda B: ((B[0], 0, inf), (B[-1], 0, inf)), _polygon_hull, halve)   # pieces: lists of floats


def levels(kind, pieces0, kn, tol, max_depth=MAX_DEPTH, sides=3, cap=CAP, s2=inf, retired=None):
    """one row of one problem: pieces0 [l] its level-0 pieces, kn [l + 1] its breaks.  sides: 1 the minimum, 2 the maximum, 3 both; s2:
    separation's threshold, a piece with plo >= s2 is not opened for the minimum; retired(B) is called with every piece whose enclosure
    goes into the result: the retired ones, and the open ones where the loop stops on them.
    Returns a dict: ext (min_lo, min_hi, max_lo, max_hi), when (t_min, t_max), which (the ends' tie-break indices), status, npieces, and for
    the tests depth (the last level evaluated), max_open (the most open pieces at a level), margin (the smallest |plo - (U - tol)| and
    |phi - (V + tol)| over every decision with a finite enclosure, for each side asked for, whether or not the other side opened the piece)
    and tie (the smaller of the figures carried with the two ends).
      ends   the smaller (larger) value is taken; of equal values the smaller time, then the smaller index.
      pole   an end without a value stops the loop after that level's end-taking, before any decision: POLE, no statement.
      NaN    a piece with a NaN is neither opened nor retired: everything NaN, status NAN (before POLE)."""
    ends, enclose, halves = kind
    kn = [float(v) for v in kn]
    hh = [kn[j + 1] - kn[j] for j in range(len(kn) - 1)]
    U, tU, wU, gU, V, tV, wV, gV = inf, inf, -1, inf, -inf, inf, -1, inf
    Rlo, Rhi = inf, -inf
    anynan = pole = False
    pieces = [(j, 0, B) for j, B in enumerate(pieces0)]
    npieces, lam, max_open, margin = 0, 0, 0, inf
    status = OK
    while True:
        npieces += len(pieces)
        for j, i, B in pieces:
            times = (kn[j] + hh[j] * (float(i) / float(1 << lam)), kn[j + 1] if i + 1 == (1 << lam) else kn[j] + hh[j] * (float(i + 1) / float(1 << lam)))
            for (v, w, fig), t in zip(ends(B), times):
                if v is None:
                    pole = True
                    continue
                if v < U or (v == U and (t < tU or (t == tU and w < wU))):
                    U, tU, wU, gU = v, t, w, fig
                if v > V or (v == V and (t < tV or (t == tV and w < wV))):
                    V, tV, wV, gV = v, t, w, fig
        opened = []
        for j, i, B in pieces:
            plo, phi = enclose(B)
            if isnan(plo) or isnan(phi):
                anynan = True
                continue
            if pole:
                continue
            if plo > -inf and phi < inf:
                if sides & 1:
                    margin = min(margin, abs(plo - (U - tol)))
                if sides & 2:
                    margin = min(margin, abs(phi - (V + tol)))
            if ((sides & 1) and plo < U - tol and not plo >= s2) or ((sides & 2) and phi > V + tol):
                opened.append((j, i, B, plo, phi))
            else:
                Rlo, Rhi = min(Rlo, plo), max(Rhi, phi)
                if retired:
                    retired(B)
        if pole:
            break
        max_open = max(max_open, len(opened))
        if not opened:
            break
        if lam == max_depth or len(opened) > cap:
            status = DEPTH if lam == max_depth else FULL
            Rlo, Rhi = min([Rlo] + [p[3] for p in opened]), max([Rhi] + [p[4] for p in opened])
            if retired:
                for p in opened:
                    retired(p[2])
            break
        pieces = []
        for j, i, B, _, _ in opened:
            L, R = halves(B)
            pieces += [(j, 2 * i, L), (j, 2 * i + 1, R)]
        lam += 1
    extra = dict(npieces=npieces, depth=lam, max_open=max_open, margin=margin, tie=min(gU, gV))
    if anynan:
        return dict(ext=(nan,) * 4, when=(nan, nan), which=(-1, -1), status=NAN, **extra)
    if pole:
        return dict(ext=(-inf, inf, -inf, inf), when=(nan, nan), which=(-1, -1), status=POLE, **extra)
    return dict(ext=(Rlo, U, V, Rhi), when=(tU, tV), which=(wU, wV), status=status, **extra)


def violation(ext, lo, up):
    """(viol [2], where [2]) of one problem from ext [nrow][4] and the rows' bounds: rule 7 of ntg_batch_extrema"""
    viol, where = [0.0, 0.0], [-1, -1]
    for side, (a, b) in enumerate(((1, 2), (0, 3))):
        for f in range(len(ext)):
            v = 0.0
            if abs(lo[f]) < INF_BOUND:
                v = max(v, lo[f] - ext[f][a])
            if abs(up[f]) < INF_BOUND:
                v = max(v, ext[f][b] - up[f])
            if v > viol[side]:
                viol[side], where[side] = v, f
    return viol, where
