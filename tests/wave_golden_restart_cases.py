"""The cases of tests/test_gpu_wave_golden_restarts.py, shared with tools/record_wave_golden.py --restarts (which records the fixture
tests/golden/wave_restarts.npz): the headline instance of sqp_wave_kernel (config M, 50 fixed majors, first 8 problems of
cf.kincar_random_bounds(3, 4096) from x = 1, identity cold start) with a quasi-Newton memory that restarts the chain right behind a
boundary of the sweep's groups of slots -- the first butterfly of pass 1 carries register slots 0 .. 15, the second slots 16 .. 19, the
third the ten LDS slots:
  qn_memory = 17   the chain grows to 17 slots: the second group never holds more than its first slot
  qn_memory = 21   20 register slots and the first LDS slot: the LDS tier never holds more than one slot
A restart empties the chain, so every length up to the memory is passed several times in 50 majors."""
import numpy as np
import torch

from ntg_amd import api, configs as cf
from wave_golden_cases import FIXED50, KEYS, NB

CASES = {
    "M_memory17_fixed50": dict(FIXED50, qn_memory=17),
    "M_memory21_fixed50": dict(FIXED50, qn_memory=21),
}


def run_case(name):
    """solve the case on cuda:0 with the loaded library; {key: numpy array} for KEYS"""
    spec = cf.config_M()
    lo, up = cf.kincar_random_bounds(3, 4096)
    lo, up = np.ascontiguousarray(lo[:NB]), np.ascontiguousarray(up[:NB])
    dev = torch.device("cuda:0")
    opts = api.default_opts(**CASES[name])
    plan = api.Plan(spec, 0)
    kernel = plan.solve_kernel(NB, opts)
    assert kernel == "sqp_wave_kernel", kernel
    x = torch.ones((NB, spec.nC), dtype=torch.float64, device=dev)
    out = plan.solve(torch.tensor(lo, device=dev), torch.tensor(up, device=dev), x, opts)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in KEYS if k != "x"}
    res["x"] = x.cpu().numpy()
    return res
