"""Quadrature rules for Plan.cost (ntg_batch_cost): (times, weights) pairs as numpy float64, [n] for one grid or [batch, n] for
per-problem grids (every row a rule of its own).  Host arithmetic only; the sums run in the library's kernel.

    t, w = quadrature.trapezoid(spec.bps)                       # the rule the solvers minimise under
    t, w = quadrature.gauss_legendre(spec.knots[0], 4)          # 4 Gauss nodes inside every knot interval
    c = plan.cost(x, torch.tensor(t, device=dev), torch.tensor(w, device=dev))["cost"]
"""
from __future__ import annotations
import numpy as np


def trapezoid(bps):
    """Nodes and weights of the plan's own rule (the reference's integrator.c on the collocation breakpoints): the breakpoints, and
    half the sum of the two intervals next to each.  bps [n] or [batch, n], n >= 2, ascending."""
    t = np.array(bps, dtype=np.float64)
    if t.ndim not in (1, 2) or t.shape[-1] < 2:
        raise ValueError("bps must be [n] or [batch, n] with n >= 2")
    h = np.diff(t, axis=-1)
    w = np.zeros_like(t)
    w[..., :-1] += h / 2
    w[..., 1:] += h / 2
    return t, w


def gauss_legendre(breaks, npts: int):
    """Composite Gauss-Legendre rule: npts nodes (numpy.polynomial.legendre.leggauss) inside every interval of `breaks`, exact for
    piecewise polynomials of degree 2 npts - 1 on them.  breaks [n] or [batch, n], ascending; returns (times, weights), each
    [(n - 1) npts] or [batch, (n - 1) npts].  Every node lies strictly inside (breaks[0], breaks[-1])."""
    br = np.asarray(breaks, dtype=np.float64)
    if br.ndim not in (1, 2) or br.shape[-1] < 2 or npts < 1:
        raise ValueError("breaks must be [n] or [batch, n] with n >= 2, and npts >= 1")
    xi, wi = np.polynomial.legendre.leggauss(npts)          # on (-1, 1), ascending
    a, b = br[..., :-1, None], br[..., 1:, None]
    h = b - a
    t = a + h * ((xi + 1.0) / 2)                            # a + positive fraction of h: never below a
    w = h * (wi / 2)
    t = t.reshape(br.shape[:-1] + (-1,))
    w = w.reshape(br.shape[:-1] + (-1,))
    # rounding may put a node of a very short interval on an end of the range: pull it one ulp inside
    lo, hi = br[..., :1], br[..., -1:]
    t = np.where(t <= lo, np.nextafter(lo, hi), t)
    t = np.where(t >= hi, np.nextafter(hi, lo), t)
    return np.ascontiguousarray(t), np.ascontiguousarray(w)
