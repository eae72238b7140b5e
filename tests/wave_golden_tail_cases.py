"""The cases of tests/test_gpu_wave_golden_tail.py, shared with tools/record_wave_golden.py --tail (which records the fixture
tests/golden/wave_tail.npz): one-wave-per-SIMD instances of sqp_wave_kernel with a SHORT or an odd-shaped tail of the direction chain in
HBM (slots from H0 = register slots + LDS slots on), the shapes the other fixtures do not reach.  Each case solves the first 8 problems
of cf.kincar_random_bounds(ncars, 4096) from x = 1 with the identity cold start for a fixed number of majors.
  M_memory31_fixed50   config M (H0 = 30), memory 31: the tail never holds more than three slots -- the odd round with its masked
                       duplicate, the carried delta of slot H0 - 1, restarts with a short tail
  M_memory34_fixed50   memory 34: a tail of up to six slots -- the HBM loop leaves at every position of its unrolled rounds
  M_memory70_fixed80   up to 80 majors, memory 70: the chain's capacity is 74 > 64 slots (more links than a wavefront has lanes),
                       44 tail slots, one restart at the capacity; the problems meet the gradient test after 73 .. 77 majors (it ends a
                       solve with a fixed number of majors too), past the restart.  (LDS: 4 waves x 4572 doubles of private area + the tables, about 157 KB of
                       the 160 KB -- the instance with ten LDS slots still fits.)
  B_fixed64            config B (two outputs, 3 doubles per lane: an odd number, the tier keeps its 8-byte layout), 64 majors: H0 = 50, a tail
                       of up to 14 slots"""
import numpy as np
import torch

from ntg_amd import api, configs as cf
from wave_golden_cases import FIXED50, KEYS, NB

# name -> (spec, cars, solve options, majors every problem runs or None)
CASES = {
    "M_memory31_fixed50": (cf.config_M, 3, dict(FIXED50, qn_memory=31), 50),
    "M_memory34_fixed50": (cf.config_M, 3, dict(FIXED50, qn_memory=34), 50),
    "M_memory70_fixed80": (cf.config_M, 3, dict(FIXED50, itlim=80, qn_memory=70), None),
    "B_fixed64": (cf.config_B, 1, dict(FIXED50, itlim=64), 64),
}


def run_case(name):
    """solve the case on cuda:0 with the loaded library; {key: numpy array} for KEYS"""
    mk, ncars, kw, _ = CASES[name]
    spec = mk()
    lo, up = cf.kincar_random_bounds(ncars, 4096)
    lo, up = np.ascontiguousarray(lo[:NB]), np.ascontiguousarray(up[:NB])
    dev = torch.device("cuda:0")
    opts = api.default_opts(**kw)
    plan = api.Plan(spec, 0)
    kernel = plan.solve_kernel(NB, opts)
    assert kernel == "sqp_wave_kernel", kernel
    x = torch.ones((NB, spec.nC), dtype=torch.float64, device=dev)
    out = plan.solve(torch.tensor(lo, device=dev), torch.tensor(up, device=dev), x, opts)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in KEYS if k != "x"}
    res["x"] = x.cpu().numpy()
    return res
