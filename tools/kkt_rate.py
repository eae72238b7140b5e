"""ntg_batch_kkt next to the evaluation it contains and to the host route it replaces.  Not a test.

On configs D and E at bench.py's batch sizes (4096 / 8192), random points and random multipliers (the work does not depend on them):

  kkt    Plan.kkt: per chunk of problems the evaluation, the expanded bounds and kkt_kernel
  eval   Plan.eval(mode 2) alone on the same batch (values, gradient, residuals, banded Jacobian rows; buffers reused)
  host   what tools/kkt.py did before: the dense Jacobian 8 problems at a time, copied to the host, r = g - A' lam_A - J' lam_c in
         numpy; measured on a sample of 64 problems and scaled to the batch

    python tools/kkt_rate.py --config D [--batch N] [--reps 9] [--calls 20] [--sample 64]

One warm-up window of each device call, then --reps alternating windows, every window --calls back-to-back calls between two device
events; prints one JSON line with the medians per call, the window-to-window spreads (max - min), the ratio kkt / eval and the scaled
host time.  Run each config as a process of its own, under its own time limit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def host_route(plan, spec, x, lam):
    """stationarity residual of every problem of x the way tools/kkt.py computed it: seconds"""
    import torch
    A = plan.tables()["A"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    worst = 0.0
    for s in range(0, x.shape[0], 8):
        ev = plan.eval(x[s:s + 8], 2, want_dense_jac=True)
        g = ev["g"].cpu().numpy(); J = ev["cJac"].cpu().numpy()
        for i in range(g.shape[0]):
            ll, ln = lam[s + i, spec.nC:spec.nC + spec.nclin], lam[s + i, spec.nC + spec.nclin:]
            worst = max(worst, np.abs(g[i] - A.T @ ll - J[i].T @ ln).max())
    return time.perf_counter() - t0, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D", choices=["D", "E"])
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--sample", type=int, default=64, help="problems the host route is measured on")
    a = ap.parse_args()
    import torch
    from ntg_amd import api, configs as cf
    if not torch.cuda.is_available():
        raise SystemExit("kkt_rate.py measures on the GPU: none found")
    spec, bounds = (cf.config_D(), cf.quadrotor_bounds) if a.config == "D" else (cf.config_E(), cf.manipulator_bounds)
    nb = a.batch or {"D": 4096, "E": 8192}[a.config]
    plan = api.Plan(spec, 0)
    rng = np.random.default_rng(1)
    ntot = spec.nC + spec.nclin + spec.ncnln
    x = torch.tensor(rng.normal(size=(nb, spec.nC)) * 0.5 + 1.0, device=DEV)
    lam_h = rng.normal(size=(nb, ntot)) * (rng.random((nb, ntot)) < 0.5)
    lam = torch.tensor(lam_h, device=DEV)
    lo, up = (torch.tensor(np.ascontiguousarray(v), device=DEV) for v in bounds(nb))

    def timed(fn):
        """ms per call over a window of --calls back-to-back calls between two device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls, r
    buf = plan.eval(x, 2)
    run_eval = lambda: plan.eval(x, 2, out=buf)
    run_kkt = lambda: plan.kkt(x, lo, up, lam)
    timed(run_kkt); timed(run_eval)   # warm-up: code objects, the allocator's pools
    tk, te = [], []
    for _ in range(max(a.reps, 5)):
        tk.append(timed(run_kkt)[0]); te.append(timed(run_eval)[0])
    res = run_kkt()["res"]
    ns = min(a.sample, nb)
    host_route(plan, spec, x[:8], lam_h)   # warm-up
    hs, worst = host_route(plan, spec, x[:ns], lam_h)
    mk, me = float(np.median(tk)), float(np.median(te))
    per = 8 * (1 + spec.nC + spec.ncnln * (1 + spec.sumk) + 2 * ntot)
    print(json.dumps(dict(config=a.config, spec=spec.name, batch=nb, calls_per_window=a.calls, kkt_ms=round(mk, 4), eval_ms=round(me, 4),
                          kkt_spread_ms=round(max(tk) - min(tk), 4), eval_spread_ms=round(max(te) - min(te), 4), kkt_over_eval=round(mk / me, 3),
                          host_sample=ns, host_sample_ms=round(1e3 * hs, 2), host_scaled_ms=round(1e3 * hs * nb / ns, 1),
                          scratch_bytes_per_problem=per, chunk=max(1, min(nb, (256 << 20) // per)),
                          sample_agrees=bool(abs(float(res[:ns, 0].max()) - worst) <= 1e-9 * max(1.0, worst)),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
