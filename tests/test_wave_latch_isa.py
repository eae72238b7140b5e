"""Static conditions of the iteration loops of the headline instance of sqp_wave_kernel (solve_wave.hpp), read from the device assembly
the build keeps.  The line search's trials repeat in a loop of their own around the evaluation site; x, gp and d do not change from
trial to trial, so its back edge moves three values.  As a `continue` of the major loop the trial's back edge shared the loop header
with the accepted step's, every carried vector had two register homes, and a trip copied them across (a latch of 68 instructions: 30
v_mov_b64, 16 v_writelane_b32, about 20 s_mov; 16 spill reloads at the head of the evaluation).  Counts of the headline instance's
body, from a compile of the commit before the loops were nested (parent) and of this tree (new), same compiler:

                                   parent   new
    .sgpr_spill_count                 136    106
    v_writelane_b32                   136    106
    v_readlane_b32                    321    254
    v_accvgpr_read_b32                441    434
    instructions                     6447   6236

The trials' latch is 11 instructions now, 3 of them moves.  The limits are the counts of this tree plus the slack the other ISA tests
use, and each is below the parent's count."""
import re

from test_wave_isa_budget import BASES, HEADLINE, _metadata
from test_wave_sweep_isa import _body

PARENT = {"sgpr_spill_count": 136, "v_writelane_b32": 136, "v_readlane_b32": 321}
LIMIT = {"sgpr_spill_count": 108, "v_writelane_b32": 108, "v_readlane_b32": 257}


def _count(body, mnemonic):
    return sum(1 for l in body if re.match(r"\s*%s\b" % mnemonic, l))


def test_limits_are_below_the_parents_counts():
    assert all(LIMIT[k] < PARENT[k] for k in PARENT)


def test_scalar_spills_of_the_headline_instance():
    md = _metadata(HEADLINE)   # (raises if the instance with 20 register slots and 10 LDS slots at base 16 is not in the object)
    assert int(md["sgpr_spill_count"]) <= LIMIT["sgpr_spill_count"], md["sgpr_spill_count"]
    assert int(md["vgpr_spill_count"]) == 0 and int(md["private_segment_fixed_size"]) == 0
    assert open(BASES).read().split() == ["16", "16"]


def test_lane_writes_and_reads_of_the_headline_instance():
    body = _body(HEADLINE)
    for mn in ("v_writelane_b32", "v_readlane_b32"):
        n = _count(body, mn)
        assert n <= LIMIT[mn], (mn, n)
