"""A/B timing of library variants on ONE box:  python tools/ab.py libA.so libB.so ...   (each in its own process; M, 4096 problems)
modes: fixed50 (headline), conv_h0 (cold start to convergence), conv_h1 (preconditioned)
Every library is run twice, alternating; a child has NTG_AB_TIMEOUT seconds (240).  The exit status is 0 when every child succeeded."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch
from ntg_amd import api, configs as cf
api.LIB_PATH = os.environ.get("NTG_AMD_LIB", api.LIB_PATH)
dev = torch.device("cuda:0")
spec = cf.config_M(); B = 4096
lo, up = cf.kincar_random_bounds(3, B)
lo = torch.tensor(lo, device=dev); up = torch.tensor(up, device=dev)
plan = api.Plan(spec, 0)
res = []
for name, opts in (("fixed50", api.default_opts(itlim=50, fixed_iters=1, hessian=0)), ("conv_h0", api.default_opts(hessian=0)), ("conv_h1", api.default_opts(hessian=1, itlim=50))):
    work = torch.empty(plan.workspace_bytes(B, opts), dtype=torch.uint8, device=dev)
    x = torch.ones((B, spec.nC), dtype=torch.float64, device=dev)
    for _ in range(3):
        x.fill_(1.0); out = plan.solve(lo, up, x, opts, work=work)
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        x.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = plan.solve(lo, up, x, opts, work=work); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    res.append(f"{name} med {ts[len(ts)//2]:.3f} min {ts[0]:.3f} ms nfev {out['nfev'].float().mean().item():.2f} F {out['objective'].sum().item():.10e}")
print(" | ".join(res))
''' % ROOT
# One child per library and repetition, each under a time limit.  A library whose child failed is not started again; after an exit that
# means a fault, an abort, a kill or a time limit NOTHING more is started: the GPU may be in a bad state, and the cause is in what was
# printed.  A GPU fault that the child met as a Python exception (exit status 1) counts as one: its text is looked for in the child's output.
FATAL = (134, 139, 124, 137)   # and every negative status (ended by a signal)
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "unspecified launch failure")
LIMIT_S = int(os.environ.get("NTG_AB_TIMEOUT", "240"))


def main(libs, reps=2):
    dropped = set()
    for rep in range(reps):
        for lib in libs:
            if lib in dropped:
                continue
            env = dict(os.environ); env["NTG_AMD_LIB"] = os.path.abspath(lib)
            try:
                r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=LIMIT_S)
                rc, text, both = r.returncode, r.stdout.strip() or r.stderr.strip()[-300:], r.stdout + r.stderr
            except subprocess.TimeoutExpired:   # (the child has been killed and reaped)
                rc, text, both = 124, "no result after %d s" % LIMIT_S, ""
            name = os.path.basename(lib)
            print(f"{name:28s} {text}", flush=True)
            fault = next((t for t in FAULT_TEXT if t in both), None)
            if rc in FATAL or rc < 0 or (rc != 0 and fault):
                why = f"exit status {rc}" + (f", '{fault}' in its output" if fault else "")
                print(f"{name:28s} {why}: a fault, an abort, a kill or a time limit -- nothing more is started", flush=True)
                return rc if rc > 1 else (128 - rc if rc < 0 else 139)
            if rc != 0:
                print(f"{name:28s} exit status {rc}: dropped from the remaining repetitions", flush=True)
                dropped.add(lib)
    return 1 if dropped else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
