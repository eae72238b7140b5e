"""Static conditions of the DPP moves of the headline instance of sqp_wave_kernel, read from the device assembly the build keeps.
A DPP move whose every lane has a source -- or whose lanes without one are to read 0 -- needs no "old" operand: with bound_ctrl the DPP
unit supplies the 0 itself, and no v_mov_b32 v, 0 is issued in front of the move.
  * from_prev / from_next (solve_wave.hpp) shift by one lane: wave_shr:1 / wave_shl:1, lane 0 / lane 63 read 0.
  * lane_xchg (wave_ops.hpp) exchanges inside a quad or a row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:8.
  * The limits of tests/test_wave_sweep_isa.py hold as they were."""
import re

from test_wave_isa_budget import HEADLINE, _metadata
from test_wave_sweep_isa import _body


def _dpp_moves(pattern):
    return [l.strip() for l in _body(HEADLINE) if re.match(r"\s*v_mov_b32_dpp\b", l) and re.search(pattern, l)]


def test_wave_shifts_fill_with_zero_themselves():
    shifts = _dpp_moves(r"\bwave_sh[lr]:1\b")
    assert len(shifts) >= 24, len(shifts)   # 12 registers each way in one trip of the evaluation loop
    bare = [l for l in shifts if "bound_ctrl" not in l]
    assert not bare, bare[:4]


def test_lane_exchanges_take_no_old_operand():
    moves = _dpp_moves(r"quad_perm:\[1,0,3,2\]|quad_perm:\[2,3,0,1\]|\brow_ror:8\b")
    assert moves, "no butterfly in the headline instance"
    bare = [l for l in moves if "bound_ctrl" not in l]
    assert not bare, bare[:4]


def test_sweep_limits_still_hold():
    md = _metadata(HEADLINE)
    assert int(md["sgpr_spill_count"]) <= 138, md["sgpr_spill_count"]
    assert int(md["vgpr_spill_count"]) == 0 and int(md["private_segment_fixed_size"]) == 0
    reads = sum(1 for l in _body(HEADLINE) if re.match(r"\s*v_accvgpr_read_b32\b", l))
    assert reads <= 2 * 20 * 12 - 4 * 12 + 11, reads
