"""What the tests, oracles and rate tools of the time certificates (Plan.envelope, Plan.envelope_sos, Plan.extrema) share: the plans and
coefficients they run on, per-problem grids for them, and the two comparisons every one of them makes."""
import dataclasses

import numpy as np

import envelope_oracle as eo
from ntg_amd import configs as cf

NSAMP = 9   # times per piece, ends included


def cpu(out):
    """a call's dict of device tensors as numpy arrays"""
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def within(got, ref, sl, label):
    """got == ref to slack where ref is finite, the same infinities elsewhere; prints the largest error in slacks"""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), label + ": the pieces without a finite bound differ"
    sl = np.broadcast_to(sl, ref.shape)
    err = np.abs(got[fin] - ref[fin]) / sl[fin]
    worst = float(err.max())
    print(f"{label}: largest error {worst:.3g} slack")
    assert worst <= 1.0, f"{label}: {worst:.3g} slack"


def piece_times(ends):
    """[npc, NSAMP] uniform times of every piece, ends included; ends [npc + 1]"""
    u = np.linspace(0.0, 1.0, NSAMP)
    t = ends[:-1, None] + (ends[1:] - ends[:-1])[:, None] * u[None, :]
    t[:, -1] = ends[1:]
    return np.clip(t, ends[0], ends[-1])


def scaled_grids(spec, scales):
    """the plan's knots scaled, every breakpoint at its own fraction of its own knot interval and, in floating point too, inside it
    (ntg_plan_set_grids wants the plan's combinatorial structure)"""
    l = spec.kninterv[0]
    k0 = np.asarray(spec.knots[0]); bp0 = np.asarray(spec.bps)
    j = np.minimum(np.searchsorted(k0, bp0, side="right") - 1, l - 1)
    fr = (bp0 - k0[j]) / (k0[j + 1] - k0[j])
    knots = np.asarray(scales)[:, None] * k0[None, :]
    bps = np.empty((len(scales), len(bp0)))
    for b, kn in enumerate(knots):
        bp = np.maximum(kn[j] + fr * (kn[j + 1] - kn[j]), kn[j])
        inner = j < l - 1
        bp[inner] = np.minimum(bp[inner], np.nextafter(kn[j + 1][inner], -np.inf))
        bp[-1] = max(bp[-1], kn[-1]) if bp0[-1] >= k0[-1] else bp[-1]
        bps[b] = bp
    return knots, bps


def greville(spec, o=0):
    k = spec.order[o]
    t = eo.aug_knots(spec.knots[o], k, spec.mult[o])
    return np.array([t[i + 1:i + k].mean() for i in range(spec.ncoef[o])])


def obstacle_x(spec, nb, seed):
    """cars that drive past the obstacle at (20, 0.5): x = 8 t and y = 0.5, both perturbed"""
    rng = np.random.default_rng(seed)
    gv = greville(spec)
    return np.concatenate([8.0 * gv[None, :] + rng.standard_normal((nb, gv.size)), 0.5 + 1.5 * rng.standard_normal((nb, gv.size))], axis=1)


def field_x(spec, lower, seed):
    """straight routes from the start to the end position of obstacle_field_problems, perturbed"""
    rng = np.random.default_rng(seed)
    f = greville(spec) / spec.knots[0][-1]
    nb = lower.shape[0]
    xs = lower[:, 0:1] + (lower[:, 6:7] - lower[:, 0:1]) * f[None, :] + 0.5 * rng.standard_normal((nb, f.size))
    ys = lower[:, 3:4] + (lower[:, 9:10] - lower[:, 3:4]) * f[None, :] + 0.5 * rng.standard_normal((nb, f.size))
    return np.concatenate([xs, ys], axis=1)


def kincar_spec():
    return cf._kincar_spec(1, 6, 3, 20, 101, 5.0, "kincar-2out-k6-l20")


def rows_spec():
    """the kincar plan with three linear trajectory rows declared inequalities: y, x' and x' - y' + 0.5 y''"""
    s = kincar_spec()
    ltc = np.zeros((3, s.nz))
    ltc[0, 3] = 1.0
    ltc[1, 1] = 1.0
    ltc[2, 1] = 1.0; ltc[2, 4] = -1.0; ltc[2, 5] = 0.5
    return dataclasses.replace(s, ltc=ltc, lin_ineq=[0] * s.nlic + [1] * 3 + [0] * s.nlfc)


def full_list_problem():
    """(spec, x [1, nC]) on 80 knot intervals with the row y: y repeats one shape on every interval (control points -2 .. 3, -0.25 at the
    knots), so every interval's polygon reaches 0.75 or more below the smallest end value"""
    spec = cf.config_O(ninterv=80)
    spec = dataclasses.replace(spec, ltc=np.eye(1, 6, 3), lin_ineq=[0] * spec.nlic + [1] + [0] * spec.nlfc)   # row 0: y
    n = spec.ncoef[0]
    return spec, np.concatenate([8.0 * greville(spec), np.array([(0.0, -2.0, 3.0)[i % 3] for i in range(n)])])[None, :]
