"""Static conditions of the pipelined chain sweep (solve_wave.hpp: sweep), read from the device assembly the build keeps.  The headline
instance keeps its 20 register slots at accumulator base 16 (its mangled name says so), spills no vector register, uses no scratch
and spills no more scalar registers than before the sweep's loads were pipelined (138); its pass 2 takes the slots kept in VGPRs
from there, so the instance holds fewer accumulator reads than two passes over 20 slots of 12 registers.
The scalar-spill bound here (138) supersedes the 150 of tests/test_wave_isa_budget.py, which stays as it was written."""
import re

from test_wave_isa_budget import ASM, HEADLINE, _metadata


def _body(name):
    lines, on = [], False
    for line in open(ASM, errors="replace"):
        if line.startswith(name + ":"):
            on = True
        elif on and line.startswith("\t.end_amdhsa_kernel"):
            break
        elif on:
            lines.append(line.split(";")[0])
    assert lines, name
    return lines


def test_headline_instance_keeps_its_budget():
    md = _metadata(HEADLINE)   # (raises if the instance with 20 register slots at base 16 is not in the object)
    assert int(md["sgpr_spill_count"]) <= 138, md["sgpr_spill_count"]
    assert int(md["vgpr_spill_count"]) == 0 and int(md["private_segment_fixed_size"]) == 0


def test_kept_slots_are_not_read_twice():
    reads = sum(1 for l in _body(HEADLINE) if re.match(r"\s*v_accvgpr_read_b32\b", l))
    # pass 2 takes R = 4 slots of 12 registers from VGPRs: 480 - 48 reads by hand, plus the few copies the register allocator parks in
    # its own accumulator registers below the base (9 today); with R = 3 the count would be 444 at the least
    assert reads <= 2 * 20 * 12 - 4 * 12 + 11, reads
