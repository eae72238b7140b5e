"""Problems of the host-callback path with outputs of mixed order, mult and maxderiv (a helper module, not a conftest).

ntg() with host callbacks is the only path where every flat output has its own order, mult, maxderiv and knot vector (DESIGN.md section 1;
every device family fixes one maxderiv for all outputs).  The cases here leave the corner the rest of the suite stays in (maxderiv 3 on every
output, one basis class, iz[o] = 3 o).  They are written as text files for tests/drivers/hostpath_drv.c, which runs them through the oracle's
ABI library (tests/test_hostpath_oracle.py, CPU) and through the product (tests/test_gpu_hostpath.py, GPU); the same Spec objects, with
family = -1 (NTG_FAM_HOST), build the oracle's tables and the product's plans.

  MIX5     evaluation: 5 outputs, orders 4,7,2,10,5, mult 1,4,0,9,3, maxderiv 1,4,2,10,3 (mult = 0, maxderiv = 1, maxderiv = order = NTG_MAX_ORDER
           at once), uneven knots per output from a seeded draw, 27 breakpoints of which four sit exactly on interior knots of outputs 0
           and 2, 3 lic + 2 ltc + 2 lfc rows with entries on every output, nonlinear rows of all three kinds, costs in all three slots, lists
           that name some but not all derivatives of an output -- the 9th derivative of the order-10 output among them
  WIDE16   evaluation: NTG_MAX_OUT = 16 outputs of maxderiv 4, nz = NTG_MAX_NZ = 64, orders alternating 5 and 6 (two basis classes), mult 3,
           4 intervals, 17 breakpoints; (15, 3) -- bit 63 of the masks, row 63 of the weighted-gradient area -- is in the trajectory cost and the
           trajectory constraint list, (0, 0) in every list
  SOLVE3   solve: 3 outputs, orders 4,6,5, mult 2,3,3, maxderiv 2,4,3, uneven knots, 19 uneven breakpoints, equality rows that pin the ends,
           cost sum_o z_o^(d_o-1)^2 + 0.1 z_o^2 + 0.5 (z_0 - z_1)^2 + 0.05 sin(z_2') with an initial and a final cost, from coef = 0.5
  SOLVE3R  solve: SOLVE3 plus the range row z_0 + 0.5 z_1' + z_2 in [LO_R, UP_R] at every breakpoint (a linear inequality row, active at the
           optimum: tests/test_hostpath_oracle.py asserts that)
  SOLVE2   solve: outputs 1 and 2 of SOLVE3 alone -- another nz, nC and row count for the driver's "sequence" mode

The solve cases carry NO nonlinear rows: the oracle does not converge on a mixed-output problem with two nonlinear rows (383 majors,
inform 4), so there would be no optimum to compare the product with.

The callbacks of the driver are one formula per function, f(u) = sum_j (a_j u_j^2 + b_j u_j) + sum w u_p u_q + sum w sin(s u_p), over the
slot's own active variables u_j.  The weights of the evaluation cases are drawn once from a seeded generator and divided by the size of
the derivative they multiply, scale(o, r) = (k-1)!/(k-1-r)! (l/T)^r: the 9th derivative of an order-10 spline is about 1e6 times its
value, and without that every figure of MIX5 would be the 9th derivative's alone.  The bilinear terms pair two outputs of different
maxderiv wherever the list has such a pair (WIDE16 has one maxderiv: different orders there).
"""
import dataclasses

import numpy as np

from ntg_amd.spec import Spec, linspace_c

FAM_HOST = -1
SLOTS = ("icav", "tcav", "fcav", "icostav", "tcostav", "fcostav")       # the order of the driver's AV and FUNCS sections


@dataclasses.dataclass
class Case:
    spec: Spec
    funcs: dict          # list name -> list of functions dict(a, b, bil [(p, q, w)], sin [(p, w, s)]) over that list
    lower: np.ndarray
    upper: np.ndarray
    coef0: np.ndarray
    points: np.ndarray   # [npts, nC]
    times: np.ndarray


def scale(spec, o, r):
    k, l, T = spec.order[o], spec.kninterv[o], float(spec.knots[o][-1] - spec.knots[o][0])
    return float(np.prod([k - 1 - i for i in range(r)])) * (l / T) ** r


def _rand_func(rng, spec, lst):
    n = len(lst)
    sc = np.array([scale(spec, o, r) for o, r in lst])
    a = rng.uniform(0.3, 1.0, n) / sc ** 2
    b = rng.normal(0.0, 0.3, n) / sc
    pairs = [(p, q) for p in range(n) for q in range(p + 1, n) if spec.maxderiv[lst[p][0]] != spec.maxderiv[lst[q][0]]]
    if not pairs:
        pairs = [(p, q) for p in range(n) for q in range(p + 1, n) if spec.order[lst[p][0]] != spec.order[lst[q][0]]]
    bil = [(p, q, float(rng.normal(0.0, 0.5) / (sc[p] * sc[q]))) for p, q in (pairs[i] for i in rng.choice(len(pairs), size=min(2, len(pairs)), replace=False))]
    p = int(rng.integers(n))
    sin = [(p, float(rng.uniform(0.2, 0.6)), float(1.0 / sc[p]))]
    return dict(a=a, b=b, bil=bil, sin=sin)


def _uneven_knots(rng, l, T):
    w = rng.uniform(0.6, 1.4, l)
    kn = T * np.concatenate([[0.0], np.cumsum(w) / w.sum()])
    kn[0] = 0.0; kn[-1] = T
    return kn


def _rows(rng, n, nz):
    return np.round(rng.normal(size=(n, nz)), 3)


def _eval_case(rng, spec, nfunc):
    funcs = {nm: [_rand_func(rng, spec, list(getattr(spec, nm))) for _ in range(nf)] for nm, nf in zip(SLOTS, nfunc)}
    lower = np.round(rng.uniform(-2.0, 0.0, spec.nbounds), 3)
    upper = lower + np.round(rng.uniform(0.0, 2.0, spec.nbounds), 3)
    points = np.stack([rng.normal(size=spec.nC), 3.0 * rng.normal(size=spec.nC), np.ones(spec.nC)])
    return funcs, lower, upper, points


def interp_times(rng, knots, T, interior2):
    """both ends, three interior knots each of outputs 0 and 2, 20 random times"""
    return np.concatenate([[0.0, T], knots[0][1:4], knots[2][interior2], rng.uniform(0.0, T, 20)])


def mix5():
    rng = np.random.default_rng(20241)
    T = 2.0
    order, mult, md, l = [4, 7, 2, 10, 5], [1, 4, 0, 9, 3], [1, 4, 2, 10, 3], [5, 3, 6, 2, 4]
    knots = [_uneven_knots(rng, li, T) for li in l]
    on_knots = [knots[0][2], knots[0][4], knots[2][1], knots[2][3]]
    while True:   # (seeded: the same draws every time) no two breakpoints closer than 0.01
        bps = np.unique(np.concatenate([[0.0, T], on_knots, rng.uniform(0.02, T - 0.02, 21)]))
        if len(bps) == 27 and np.diff(bps).min() > 1e-2:
            break
    assert all(t in bps for t in on_knots)
    nz = sum(md)
    spec = Spec(nout=5, bps=bps, kninterv=l, knots=knots, order=order, mult=mult, maxderiv=md, family=FAM_HOST,
                lic=_rows(rng, 3, nz), ltc=_rows(rng, 2, nz), lfc=_rows(rng, 2, nz), nnlic=1, nnltc=2, nnlfc=1,
                icav=[(0, 0), (1, 1), (2, 1), (3, 9), (4, 0)],
                tcav=[(0, 0), (1, 0), (1, 3), (2, 0), (3, 4), (3, 9), (4, 2)],
                fcav=[(1, 2), (2, 1), (3, 0), (3, 8), (4, 1)],
                nicf=1, nucf=1, nfcf=1,
                icostav=[(0, 0), (1, 0), (1, 2), (2, 0), (3, 1), (3, 9), (4, 1)],
                tcostav=[(0, 0), (1, 1), (1, 3), (2, 1), (3, 0), (3, 5), (3, 9), (4, 0), (4, 2)],
                fcostav=[(0, 0), (1, 3), (2, 0), (3, 2), (3, 9), (4, 2)], name="MIX5")
    funcs, lower, upper, points = _eval_case(rng, spec, (1, 2, 1, 1, 1, 1))
    return Case(spec, funcs, lower, upper, np.ones(spec.nC), points, interp_times(rng, knots, T, [1, 3, 5]))


def wide16():
    rng = np.random.default_rng(20242)
    T, nout = 2.0, 16
    order = [5, 6] * 8
    knots = [linspace_c(0.0, T, 5) for _ in range(nout)]
    tcost = sorted({(0, 0), (15, 3)} | {(o, o % 4) for o in range(nout)} | {(o, (o + 2) % 4) for o in range(nout)})
    spec = Spec(nout=nout, bps=linspace_c(0.0, T, 17), kninterv=[4] * nout, knots=knots, order=order, mult=[3] * nout, maxderiv=[4] * nout,
                family=FAM_HOST, ltc=_rows(rng, 1, 64), nnlic=1, nnltc=1, nnlfc=1,
                icav=[(0, 0), (6, 3), (15, 2)], tcav=[(0, 0), (3, 1), (7, 2), (8, 0), (12, 3), (14, 1), (15, 3)], fcav=[(0, 0), (2, 2), (11, 0), (15, 3)],
                nicf=1, nucf=1, nfcf=1,
                icostav=[(0, 0), (5, 2), (10, 1), (15, 0)], tcostav=tcost, fcostav=[(0, 0), (4, 3), (9, 1), (15, 3)], name="WIDE16")
    assert spec.nz == 64
    funcs, lower, upper, points = _eval_case(rng, spec, (1, 1, 1, 1, 1, 1))
    return Case(spec, funcs, lower, upper, np.ones(spec.nC), points, interp_times(rng, knots, T, [1, 2, 3]))


# the range of SOLVE3R's row: at SOLVE3's optimum the row rises from -0.75 (t = 0, pinned) to 0.622 at breakpoint 11 and falls to 0.4 (t = T,
# pinned: z_1'(T) = -2 is what makes it fall).  [-0.8, 0.615] leaves both pinned ends feasible and cuts the top off: one row at its upper
# bound, the objective 6.9e-6 above SOLVE3's, the oracle at inform 0 after 124 (default) and 36 (colloc) of at most 180 majors.  Tighter
# ranges take the default mode to the iteration limit (0.5: inform 4); tests/test_hostpath_oracle.py asserts what the choice has to give.
LO_R, UP_R = -0.8, 0.615


def _solve_case(outputs, range_row):
    T = 2.0
    rng = np.random.default_rng(20243)
    order3, mult3, md3, l3 = [4, 6, 5], [2, 3, 3], [2, 4, 3], [4, 3, 4]
    knots3 = [_uneven_knots(rng, li, T) for li in l3]
    u = np.arange(19) / 18.0
    bps = T * (u + 0.25 * u * (1.0 - u)); bps[0] = 0.0; bps[-1] = T
    sel = list(outputs); new = {o: i for i, o in enumerate(sel)}
    md = [md3[o] for o in sel]; nz = sum(md); iz = np.concatenate([[0], np.cumsum(md)])[:-1]

    def av(lst):
        return [(new[o], r) for o, r in lst if o in new]

    def row(entries):
        v = np.zeros(nz)
        for (o, r), w in entries.items():
            if o in new:
                v[iz[new[o]] + r] = w
        return v
    pins_i = {(0, 0): -0.5, (1, 0): 0.3, (1, 1): -0.5, (2, 0): 0.0}
    pins_f = {(0, 0): 0.8, (1, 0): -0.4, (1, 1): -2.0, (2, 0): 0.6}
    lic = np.array([row({k: 1.0}) for k in pins_i if k[0] in new]); lo_i = [v for k, v in pins_i.items() if k[0] in new]
    lfc = np.array([row({k: 1.0}) for k in pins_f if k[0] in new]); lo_f = [v for k, v in pins_f.items() if k[0] in new]
    ltc = np.array([row({(0, 0): 1.0, (1, 1): 0.5, (2, 0): 1.0})]) if range_row else np.zeros((0, nz))
    tcost = av([(0, 0), (0, 1), (1, 0), (1, 3), (2, 0), (2, 1), (2, 2)])
    icost = av([(1, 2), (2, 1)]); fcost = av([(0, 1), (1, 1), (2, 2)])
    spec = Spec(nout=len(sel), bps=bps, kninterv=[l3[o] for o in sel], knots=[knots3[o] for o in sel], order=[order3[o] for o in sel],
                mult=[mult3[o] for o in sel], maxderiv=md, family=FAM_HOST, lic=lic, ltc=ltc, lfc=lfc,
                nicf=1, nucf=1, nfcf=1, icostav=icost, tcostav=tcost, fcostav=fcost,
                name="SOLVE" + "".join(str(o) for o in sel) + ("R" if range_row else ""))

    def func(lst, quad, bil, sin):
        idx = {k: j for j, k in enumerate(lst)}
        a = np.zeros(len(lst))
        for k, w in quad.items():
            if (new.get(k[0]), k[1]) in idx:
                a[idx[(new[k[0]], k[1])]] += w
        nk = lambda k: (new.get(k[0]), k[1])
        return dict(a=a, b=np.zeros(len(lst)),
                    bil=[(idx[nk(p)], idx[nk(q)], w) for p, q, w in bil if nk(p) in idx and nk(q) in idx],
                    sin=[(idx[nk(p)], w, s) for p, w, s in sin if nk(p) in idx])
    # sum_o z_o^(d_o - 1)^2 + 0.1 z_o^2, + 0.5 (z_0 - z_1)^2 = 0.5 z_0^2 - z_0 z_1 + 0.5 z_1^2, + 0.05 sin(z_2')
    quad = {(0, 1): 1.0, (1, 3): 1.0, (2, 2): 1.0, (0, 0): 0.1, (1, 0): 0.1, (2, 0): 0.1}
    both = 0 in new and 1 in new
    if both:
        quad[(0, 0)] += 0.5; quad[(1, 0)] += 0.5
    funcs = {nm: [] for nm in SLOTS}
    funcs["tcostav"] = [func(tcost, quad, [((0, 0), (1, 0), -1.0)], [((2, 1), 0.05, 1.0)])]
    funcs["icostav"] = [func(icost, {(1, 2): 0.3, (2, 1): 0.2}, [((1, 2), (2, 1), 0.1)], [((2, 1), 0.05, 1.0)])]
    funcs["fcostav"] = [func(fcost, {(0, 1): 0.4, (1, 1): 0.3, (2, 2): 0.2}, [((0, 1), (2, 2), 0.1), ((1, 1), (2, 2), 0.1)], [((1, 1), 0.05, 1.0)])]
    lower = np.array(lo_i + ([LO_R] if range_row else []) + lo_f); upper = np.array(lo_i + ([UP_R] if range_row else []) + lo_f)
    return Case(spec, funcs, lower, upper, np.full(spec.nC, 0.5), np.zeros((0, spec.nC)), np.zeros(0))


CASES = {"MIX5": mix5, "WIDE16": wide16, "SOLVE3": lambda: _solve_case((0, 1, 2), False), "SOLVE3R": lambda: _solve_case((0, 1, 2), True),
         "SOLVE2": lambda: _solve_case((1, 2), False)}
HESSIAN_MODES = {"default": (), "colloc": ("hessian colloc",)}          # the two modes the solve cases run in: npsoloption strings


def write(case, path, points=None, full=None):
    """the problem file of tests/drivers/hostpath_drv.c; points [npts, nC] (default: the case's), full [npts] flags (default: all 1)"""
    sp = case.spec
    pts = case.points if points is None else np.asarray(points)
    full = np.ones(len(pts), dtype=int) if full is None else np.asarray(full, dtype=int)
    num = lambda v: " ".join("%.17g" % x for x in np.asarray(v, dtype=float).ravel())
    out = ["NOUT %d" % sp.nout]
    for o in range(sp.nout):
        out.append("%d %d %d %d %s" % (sp.order[o], sp.mult[o], sp.maxderiv[o], sp.kninterv[o], num(sp.knots[o])))
    out.append("BPS %d %s" % (sp.nbps, num(sp.bps)))
    for key, M in (("LIC", sp.lic), ("LTC", sp.ltc), ("LFC", sp.lfc)):
        out.append("%s %d %s" % (key, M.shape[0], num(M)))
    out.append("AV")
    for nm in SLOTS:
        lst = list(getattr(sp, nm))
        out.append("%d %s" % (len(lst), " ".join("%d %d" % av for av in lst)))
    out.append("NFUNC %d %d %d %d %d %d" % (sp.nnlic, sp.nnltc, sp.nnlfc, sp.nicf, sp.nucf, sp.nfcf))
    out.append("BOUNDS %d %s %s" % (sp.nbounds, num(case.lower), num(case.upper)))
    out.append("FUNCS")
    for nm in SLOTS:
        for f in case.funcs[nm]:
            out.append("%s %s" % (num(f["a"]), num(f["b"])))
            out.append("%d %s" % (len(f["bil"]), " ".join("%d %d %.17g" % t for t in f["bil"])))
            out.append("%d %s" % (len(f["sin"]), " ".join("%d %.17g %.17g" % t for t in f["sin"])))
    out.append("COEF %d %s" % (sp.nC, num(case.coef0)))
    out.append("POINTS %d" % len(pts))
    for fl, x in zip(full, pts):
        out.append("%d %s" % (fl, num(x)))
    out.append("TIMES %d %s" % (len(case.times), num(case.times)))
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return path


def parse_eval(text, case):
    """the driver's eval output: a list with one dict per point (F, G, F0, G1, C, J [ldJ, nC], Z [P, ntcostav], INTERP {o: [ntimes, d_o]}, C0)"""
    sp = case.spec
    pts, cur, shape = [], None, None
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "SHAPE":
            shape = [int(v) for v in w[1:]]
        elif w[0] == "POINT":
            cur = dict(full=int(w[2]), Z={}, INTERP={}); pts.append(cur)
        elif w[0] in ("F", "F0"):
            cur[w[0]] = float(w[1])
        elif w[0] in ("G", "G1", "C", "C0"):
            cur[w[0]] = np.array(w[1:], dtype=float)
        elif w[0] == "J":
            cur["J"] = np.array(w[1:], dtype=float).reshape(sp.nC, shape[2]).T      # column-major ldJ x nC
        elif w[0] == "Z":
            cur["Z"][int(w[1])] = np.array(w[2:], dtype=float)
        elif w[0] == "INTERP":
            cur["INTERP"][(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=float)
    assert shape is not None and shape[0] == sp.nC and shape[1] == sp.ncnln and shape[2] == sp.ncnln + 2, shape
    for p in pts:
        if p["Z"]:
            p["Z"] = np.stack([p["Z"][i] for i in range(sp.nbps)])
        if p["INTERP"]:
            p["INTERP"] = {o: np.stack([p["INTERP"][(o, t)] for t in range(len(case.times))]) for o in range(sp.nout)}
    return pts


def parse_solve(text):
    """the driver's solve / sequence output: one dict(inform, objective, x, istate) per ntg() call"""
    res = [np.array(l.split()[1:], dtype=float) for l in text.splitlines() if l.startswith("RESULT")]
    ist = [[int(v) for v in l.split()[1:]] for l in text.splitlines() if l.startswith("ISTATE")]
    assert len(res) == len(ist)
    return [dict(inform=int(r[0]), objective=r[1], x=r[2:], istate=i) for r, i in zip(res, ist)]
