"""Static conditions of the norms and of the |g|^2 sum in the headline instance of sqp_wave_kernel (solve_wave.hpp), read from the device
assembly the build keeps.  The square roots of the totals that come out of the 16-wide butterflies are taken in lanes before the
broadcasts (one root sequence for |s|, |y|, |x|, |gp+| of an accepted step, one for |x|, |gp| of the first major; after the
broadcasts each total had a sequence of its own, on 64 identical lanes), and |g|^2, which only the tolerance tolg reads, is not summed at
the evaluation site: that sum carries two values (the quadrature and the slope), and |g|^2 of an accepted point rides with the two
products of the new direction; tolg is formed behind the tests that read it, not at the top of every major.  Counts of the headline
instance's body, from a compile of the commit before (parent) and of this tree (new), same compiler:

                                          parent   new
    instructions                            6236   6183
    v_rsq_f64                                 14     10
    row_ror:1 moves, evaluation to the
      inner loop's back edge                   6      4

(v_rsq_f64 counts root sequences in the text, not executions: per accepted major the fixed-work solve runs two of them where it ran
five -- one in lanes for the four norms of an accepted step, one for |d|.)  The limits are the counts of this tree plus the slack the
other ISA tests use, and each is below the parent's count; the rotations are asserted as a number, two per summed value."""
import re

from test_wave_isa_budget import ASM, HEADLINE

PARENT = {"instructions": 6236, "v_rsq_f64": 14, "row_ror:1": 6}
LIMIT = {"instructions": 6230, "v_rsq_f64": 11}


def _blocks(name, asm=None):
    """the kernel's basic blocks in layout order: [label, lines without comments]"""
    blocks, on = [["", []]], False
    for line in open(asm or ASM, errors="replace"):
        if line.startswith(name + ":"):
            on = True
        elif on and line.startswith("\t.end_amdhsa_kernel"):
            break
        elif on:
            m = re.match(r"(\.LBB\d+_\d+):", line)
            if m:
                blocks.append([m.group(1), []])
            else:
                blocks[-1][1].append(line.split(";")[0])
    assert len(blocks) > 1, name
    return blocks


def _is_instruction(line):
    return re.match(r"\s+[a-z]\w*", line) is not None and not line.strip().startswith(".")


def _count(blocks, what):
    return sum(1 for _, ls in blocks for l in ls if what in l)


def evaluation_to_back_edge(blocks):
    """the block of the evaluation -- the one with the cluster of ds_read of the interval tables, next to the DPP shift that fetches the
    next lane's coefficients (wave_shl:1) -- and the blocks behind it up to the last branch back to it: the inner loop's back edge"""
    ev = [i for i, (_, ls) in enumerate(blocks) if sum("ds_read" in l for l in ls) >= 20 and any("wave_shl:1" in l for l in ls)]
    assert len(ev) == 1, ev
    label = blocks[ev[0]][0]
    back = [i for i, (_, ls) in enumerate(blocks) if i >= ev[0] and any(re.match(r"\s*s_c?branch\w*\s+%s\s*$" % re.escape(label), l) for l in ls)]
    assert back, "no branch back to the evaluation block"
    return blocks[ev[0]:back[-1] + 1]


def test_limits_are_below_the_parents_counts():
    assert all(LIMIT[k] < PARENT[k] for k in LIMIT)


def test_instructions_and_root_sequences_of_the_headline_instance():
    blocks = _blocks(HEADLINE)
    n = sum(1 for _, ls in blocks for l in ls if _is_instruction(l))
    assert n <= LIMIT["instructions"], n
    r = _count(blocks, "v_rsq_f64")
    assert r <= LIMIT["v_rsq_f64"], r


def test_evaluation_site_sums_two_values():
    region = evaluation_to_back_edge(_blocks(HEADLINE))
    # wave_sums_few: one row_ror:1 move per half of a double, so two per value -- the quadrature and the slope; |g|^2 was the third
    assert _count(region, "row_ror:1") == 4, _count(region, "row_ror:1")
