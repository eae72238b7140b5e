"""-m gpu: the headline workload's kernel (sqp_wave_kernel, FAT instance) reproduces a recorded result bit for bit.  The first 64
problems of the bench batch (config M, the bench's bounds stream, identity cold start, exactly 50 SQP majors) are solved and compared
with tests/golden/wave_m_fixed50_64.npz: coefficients, objective, inform, iterations and evaluation counts.  Register-allocation
and scheduling work on that kernel must not move a single bit of its results; this test says so directly."""
import os

import numpy as np
import pytest
import torch

from ntg_amd import api, configs as cf
from gpu_common import dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_m_fixed50_64.npz")


def test_fixed_50_majors_bitwise():
    ref = np.load(GOLDEN)
    spec = cf.config_M()
    lo, up = cf.kincar_random_bounds(3, 4096)   # the bench's problem stream; its first 64 problems
    lo, up = lo[:64], up[:64]
    plan = api.Plan(spec, 0)
    opts = api.default_opts(itlim=50, fixed_iters=1, hessian=0)
    assert plan.solve_kernel(64, opts) == "sqp_wave_kernel"
    x = torch.ones((64, spec.nC), dtype=torch.float64, device="cuda:0")
    out = plan.solve(dev(lo), dev(up), x, opts)
    torch.cuda.synchronize()
    assert np.array_equal(out["iters"].cpu().numpy(), ref["iters"])
    assert np.array_equal(out["nfev"].cpu().numpy(), ref["nfev"])
    assert np.array_equal(out["inform"].cpu().numpy(), ref["inform"])
    # bitwise: compare the bit patterns (array_equal on floats would also accept -0.0 == 0.0)
    assert np.array_equal(out["objective"].cpu().numpy().view(np.int64), ref["objective"].view(np.int64))
    assert np.array_equal(x.cpu().numpy().view(np.int64), ref["x"].view(np.int64))
