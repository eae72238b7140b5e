"""Static conditions of the HBM tier of the chain sweep (solve_wave.hpp: slot_store, hload), read from the device assembly the build keeps.
On the one-wave-per-SIMD instances with an even number of doubles per lane a slot of the tier is stored [EPL/2][lane][2], so a slot
moves in three 16-byte requests per lane instead of six 8-byte ones.  Counts of the headline instance's body, from a compile of the
commit before the layout changed (parent) and of this tree (new), same compiler:

                                   parent   new
    lines                            8436   8403
    global_load_dwordx4                 2     20
    global_load_dwordx2                63     27
    global_store_dwordx4                2      5
    global_store_dwordx2               10      4
    ds_read_b64 + ds_read2_b64    60 + 28   60 + 28
    v_accvgpr_read_b32                441    441
    .sgpr_spill_count                 136    136

The 8-byte LDS reads are those of the sweep's scalars (links, deltas); moving those into lanes was measured and not kept,
so their count is held where it was, not lowered.  The limits of tests/test_wave_isa_budget.py, tests/test_wave_sweep_isa.py and
tests/test_wave_butterfly_isa.py are restated: the layout must not have cost the instance its register budget."""
import re

from test_wave_isa_budget import BASES, HEADLINE, _metadata
from test_wave_sweep_isa import _body


def _count(body, *mnemonics):
    return sum(1 for l in body if re.match(r"\s*(%s)\b" % "|".join(mnemonics), l))


def test_tail_moves_in_16_byte_requests():
    body = _body(HEADLINE)
    x4, x2 = _count(body, "global_load_dwordx4"), _count(body, "global_load_dwordx2")
    # two rounds of two slots in the loop, the first round ahead of the on-chip passes: at least 3 x 2 x 3 requests of 16 bytes
    assert x4 >= 18, x4
    assert x2 < 63, x2
    assert _count(body, "global_store_dwordx4") >= 3   # slot_store of one slot


def test_sweep_scalars_read_no_more_than_before():
    body = _body(HEADLINE)
    assert _count(body, "ds_read_b64", "ds_read2_b64") <= 88


def test_budgets_of_the_headline_instance_hold():
    assert open(BASES).read().split() == ["16", "16"]
    md = _metadata(HEADLINE)   # (raises if the instance with 20 register slots and 10 LDS slots at base 16 is not in the object)
    assert int(md["sgpr_spill_count"]) <= 138, md["sgpr_spill_count"]
    assert int(md["vgpr_spill_count"]) == 0 and int(md["private_segment_fixed_size"]) == 0
    assert _count(_body(HEADLINE), "v_accvgpr_read_b32") <= 443
