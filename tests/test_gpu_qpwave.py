"""-m gpu: the passive-set solve sqp_kernel runs in the QP-based SQP step (csrc/qpdual.hpp, qp_passive_solve_wave: all lanes of the group's
wave) against its specification, the scalar qp_passive_solve the host test exercises (tests/test_oracle_qpsqp.py), on the same slots.
tests/drivers/qpwave_unit.hip: one workgroup runs the wave routine, one lane the scalar routine on a copy.  Working sets of 1, 2, 15, 16
(16 slots per group) and 31, 32 slots (32 per group), S = G G'/m + I (condition number at most about 1e3), random signs and right-hand
sides.  The seeds were chosen on the CPU (qpwave_unit choose): no decision of the ratio test or the drop rule within 1e-6 of a tie --
the driver checks that again before it runs anything -- and on at least two seeds per size slots leave the passive set.
Asserted (by the driver's exit status): the same passive set exactly, and max_a |nu_a - nu'_a| <= 1e-10 max_a |nu_a|: relative to the
largest multiplier, not entry by entry -- the error of a Cholesky solve is bounded in the norm of the solution, and an entry small against
the largest carries the absolute error of the large ones.  The two Cholesky orders differ by about cond x np x 2^-53 = 4e-12 in that
norm, the bound leaves 25 times that."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def unit_exe():
    src = os.path.join(HERE, "drivers", "qpwave_unit.hip"); exe = os.path.join(HERE, "drivers", "qpwave_unit")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(HERE, "..", "include"),
                               "-Wno-unused-value", "-Wno-pass-failed", "-o", exe, src], cwd=os.path.join(HERE, "drivers"))
    return exe


# (slots, seed, slots that leave the passive set)
@pytest.mark.parametrize("ns,seed,leave", [(1, 2, 0), (1, 1, 1), (1, 4, 1), (2, 3, 1), (2, 5, 2), (2, 6, 2), (15, 3, 4), (15, 10, 9), (16, 5, 7), (16, 3, 9),
                                           (31, 5, 17), (31, 9, 12), (32, 4, 15), (32, 1, 15), (32, 11, 16)])
def test_wave_solve_is_the_scalar_solve(unit_exe, ns, seed, leave):
    r = subprocess.run([unit_exe, str(ns), str(seed)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(re.search(r": (\d+) slots leave", r.stdout).group(1)) == leave
