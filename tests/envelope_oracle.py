"""An independent statement of ntg_batch_envelope's definition (include/ntg_amd.h) in numpy / scipy, for the tests.

The interval polygons are NOT built by the blossom the kernel uses: the spline goes into scipy.interpolate.BSpline, the polynomial of
every knot interval is taken from it (a BSpline on that span's own 2k knots and k coefficients: the same polynomial, defined at both
ends of the interval), and its Bernstein coefficients come from solving the Bernstein collocation system at k Chebyshev points of
the interval.  Differences, cuts (the blossom of the polygon at the piece's ends, argument by argument) and degree elevation follow in
plain numpy.
"""
import numpy as np
from scipy.interpolate import BSpline
from scipy.special import comb

SLACK = 2.0 ** -42


def aug_knots(brk, k, m):
    """first / last break k times, interior breaks k - m times"""
    brk = np.asarray(brk, dtype=np.float64)
    return np.concatenate([[brk[0]] * k, np.repeat(brk[1:-1], k - m), [brk[-1]] * k])


def interval_spline(brk, k, m, c, j):
    """the polynomial of knot interval j as a BSpline on the span's own knots: c [n] or [nb, n]"""
    t = aug_knots(brk, k, m)
    mu = k - 1 + j * (k - m)
    cc = np.atleast_2d(np.asarray(c, dtype=np.float64))[:, mu - k + 1:mu + 1]
    return BSpline(t[mu - k + 1:mu + k + 1], cc.T, k - 1, extrapolate=True)


def bernstein(d, s):
    """[len(s), d + 1]: B_{i,d}(s)"""
    s = np.asarray(s, dtype=np.float64)[:, None]
    i = np.arange(d + 1)[None, :]
    return comb(d, i) * s ** i * (1.0 - s) ** (d - i)


def interval_polygons(brk, k, m, c):
    """Bezier control points of z on every knot interval: [nb, l, k]"""
    brk = np.asarray(brk, dtype=np.float64)
    c = np.atleast_2d(c)
    l = len(brk) - 1
    s = 0.5 - 0.5 * np.cos((2 * np.arange(k) + 1) * np.pi / (2 * k))   # Chebyshev points of [0, 1]
    M = bernstein(k - 1, s)
    out = np.empty((c.shape[0], l, k))
    for j in range(l):
        v = interval_spline(brk, k, m, c, j)(brk[j] + (brk[j + 1] - brk[j]) * s)   # [k, nb]
        out[:, j, :] = np.linalg.solve(M, v).T
    return out


def difference(B, h):
    """polygon of the derivative: B [..., l, d + 1], h [l] -> [..., l, d]"""
    d = B.shape[-1] - 1
    return d / np.asarray(h)[:, None] * (B[..., 1:] - B[..., :-1])


def cut(B, s0, s1):
    """polygon on [s0, s1] of the local parameter: control point i is the blossom at (s0 x (d - i), s1 x i)"""
    d = B.shape[-1] - 1
    out = np.empty_like(B)
    for i in range(d + 1):
        P = B
        for u in [s0] * (d - i) + [s1] * i:
            P = (1.0 - u) * P[..., :-1] + u * P[..., 1:]
        out[..., i] = P[..., 0]
    return out


def elevate(B):
    d = B.shape[-1] - 1
    out = np.empty(B.shape[:-1] + (d + 2,))
    out[..., 0] = B[..., 0]; out[..., d + 1] = B[..., d]
    for i in range(1, d + 1):
        a = i / (d + 1)
        out[..., i] = a * B[..., i - 1] + (1.0 - a) * B[..., i]
    return out


def piece_polygons(brk, k, m, c, nder, nsub):
    """list over r < min(nder, k) of [nb, l << nsub, k - r]: the control points of D^r z on every piece"""
    brk = np.asarray(brk, dtype=np.float64)
    B = interval_polygons(brk, k, m, c)
    n = 1 << nsub
    out = []
    for r in range(min(nder, k)):
        if r > 0:
            B = difference(B, np.diff(brk))
        P = np.stack([cut(B, i / n, (i + 1) / n) for i in range(n)], axis=2)   # [nb, l, n, d + 1]
        out.append(P.reshape(P.shape[0], -1, P.shape[-1]))
    return out


def hull(P):
    """min and max over the control points; a NaN among them stays"""
    return np.min(P, axis=-1), np.max(P, axis=-1)


def coef_slices(spec):
    off = np.concatenate([[0], np.cumsum(spec.ncoef)])
    return [slice(off[o], off[o + 1]) for o in range(spec.nout)]


def flag_index(spec):
    return np.concatenate([[0], np.cumsum(spec.maxderiv)])


def slack(spec, x, knots=None):
    """[nb, nz]: 2^-42 max_i |c_{o,i}| (2 (k - 1) / h_min)^r for entry iz[o] + r"""
    x = np.atleast_2d(x)
    out = np.zeros((x.shape[0], spec.nz))
    iz = flag_index(spec)
    for o, sl in enumerate(coef_slices(spec)):
        hmin = np.diff(np.asarray(spec.knots[o] if knots is None else knots)).min()
        cm = np.abs(x[:, sl]).max(axis=1)
        for r in range(spec.maxderiv[o]):
            out[:, iz[o] + r] = SLACK * cm * (2.0 * (spec.order[o] - 1) / hmin) ** r
    return out


def entry_envelope(spec, x, nsub, knots=None):
    """lo, hi [nb, nz, npc] of the definition; knots: one break sequence for every output instead of the spec's (per-problem grids)"""
    x = np.atleast_2d(x)
    npc = max(spec.kninterv) << nsub
    lo = np.full((x.shape[0], spec.nz, npc), np.inf); hi = np.full_like(lo, -np.inf)
    iz = flag_index(spec)
    for o, sl in enumerate(coef_slices(spec)):
        brk = spec.knots[o] if knots is None else knots
        n = spec.kninterv[o] << nsub
        polys = piece_polygons(brk, spec.order[o], spec.mult[o], x[:, sl], spec.maxderiv[o], nsub)
        for r in range(spec.maxderiv[o]):
            if r < len(polys):
                lo[:, iz[o] + r, :n], hi[:, iz[o] + r, :n] = hull(polys[r])
            else:
                lo[:, iz[o] + r, :n] = hi[:, iz[o] + r, :n] = 0.0
    return lo, hi


def row_envelope(spec, x, nsub, knots=None):
    """row_lo, row_hi [nb, nltc, npc]: every named entry's polygon elevated to the row's largest degree, summed with the row's coefficients"""
    x = np.atleast_2d(x)
    ltc = np.asarray(spec.ltc, dtype=np.float64).reshape(spec.nltc, spec.nz)
    npc = max(spec.kninterv) << nsub
    lo = np.full((x.shape[0], spec.nltc, npc), np.inf); hi = np.full_like(lo, -np.inf)
    iz = flag_index(spec)
    sls = coef_slices(spec)
    polys = {}
    for i in range(spec.nltc):
        named = [(o, r) for o in range(spec.nout) for r in range(min(spec.maxderiv[o], spec.order[o])) if ltc[i, iz[o] + r] != 0.0]
        o0 = named[0][0] if named else 0
        assert all(spec.order[o] == spec.order[o0] and spec.kninterv[o] == spec.kninterv[o0] and spec.mult[o] == spec.mult[o0] and
                   np.array_equal(spec.knots[o], spec.knots[o0]) for o, _ in named), "the row names outputs of different basis classes"
        n = spec.kninterv[o0] << nsub
        if not named:
            lo[:, i, :n] = hi[:, i, :n] = 0.0
            continue
        D = max(spec.order[o] - 1 - r for o, r in named)
        S = 0.0
        for o, r in named:   # v ascending
            if o not in polys:
                polys[o] = piece_polygons(spec.knots[o] if knots is None else knots, spec.order[o], spec.mult[o], x[:, sls[o]], spec.maxderiv[o], nsub)
            P = polys[o][r]
            while P.shape[-1] - 1 < D:
                P = elevate(P)
            S = S + ltc[i, iz[o] + r] * P
        lo[:, i, :n], hi[:, i, :n] = hull(S)
    return lo, hi


def row_slack(spec, x, knots=None):
    """[nb, nltc]: sum_v |ltc[i][v]| slack_v -- the row's polygon is that combination of the entries' polygons"""
    ltc = np.abs(np.asarray(spec.ltc, dtype=np.float64).reshape(spec.nltc, spec.nz))
    return slack(spec, x, knots) @ ltc.T


def violation(spec, row_lo, row_hi, lower, upper, inf_bound=1e20):
    """viol [nb], where [nb, 2] of the definition"""
    nb, nltc, npc = row_lo.shape
    viol = np.zeros(nb); where = np.full((nb, 2), -1, dtype=np.int64)
    for b in range(nb):
        v = np.zeros((nltc, npc))
        for i in range(nltc):
            l, u = lower[b, spec.nlic + i], upper[b, spec.nlic + i]
            live = np.isfinite(row_lo[b, i]) | np.isnan(row_lo[b, i])
            if abs(l) < inf_bound:
                v[i] = np.maximum(v[i], np.where(live, l - row_lo[b, i], 0.0))
            if abs(u) < inf_bound:
                v[i] = np.maximum(v[i], np.where(live, row_hi[b, i] - u, 0.0))
        if v.max() > 0:
            viol[b] = v.max()
            where[b] = divmod(int(np.argmax(v)), npc)   # the first of equal maxima
    return viol, where


def sample_piece(brk, k, m, c, r, nsub, nsamp):
    """D^r z at nsamp uniform local parameters of every piece, ends included: [nb, l << nsub, nsamp], from the interval's own polynomial"""
    brk = np.asarray(brk, dtype=np.float64)
    c = np.atleast_2d(c)
    l, n = len(brk) - 1, 1 << nsub
    out = np.empty((c.shape[0], l * n, nsamp))
    u = np.linspace(0.0, 1.0, nsamp)
    for j in range(l):
        sp = interval_spline(brk, k, m, c, j)
        for i in range(n):
            s = np.clip((i + u) / n, 0.0, 1.0)
            t = brk[j] + (brk[j + 1] - brk[j]) * s
            t[0] = brk[j] if i == 0 else t[0]; t[-1] = brk[j + 1] if i == n - 1 else t[-1]
            out[:, j * n + i, :] = (sp(t, nu=r) if r < k else np.zeros((nsamp, c.shape[0]))).T
    return out
