"""Register budget of the headline kernel, read from the device assembly the build keeps (ntg_amd/build.py compiles
fam_kincar_wave.hip with -save-temps and audits it).  The FAT instance of sqp_wave_kernel that bench.py measures runs one wave per
SIMD and is bound by instruction issue: every scalar register it spills costs a v_writelane / v_readlane pair (VALU instructions) plus
wait states wherever the value is used.  This test holds the line reached by reading kernel arguments at their point of use and
forming lane masks where they are needed (214 spilled scalar registers before, 138 after), and checks that the build kept the full
register tier of the chain (accumulator bases 16 / 16: the ISA audit did not have to raise them)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntg_amd", "csrc")
ASM = os.path.join(CSRC, "fam_kincar_wave-hip-amdgcn-amd-amdhsa-gfx950.s")
BASES = os.path.join(CSRC, "fam_kincar_wave.abase")
# sqp_wave_kernel<NTG_FAM_KINCAR, 6, 2, 6, 4, 20, 4, 1, 20, 10, false, false, false, 16>: config M, 50 fixed majors (bench.py)
HEADLINE = "_ZN4ntgw15sqp_wave_kernelILi0ELi6ELi2ELi6ELi4ELi20ELi4ELi1ELi20ELi10ELb0ELb0ELb0ELi16EEEv7NtgDims9NtgTables11SolveParamsNS_8WaveArgsE"
SGPR_SPILL_MAX = 150


def _metadata(name):
    """the kernel's entry in the code object metadata (.amdgpu_metadata) as {key: value}"""
    fields, cur = {}, None
    for line in open(ASM, errors="replace"):
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name":
            if cur == name:
                break
            cur, fields = val, {}
        elif cur == name:
            fields[key] = val
            if key == "wavefront_size":   # the last key of an entry
                break
    assert cur == name, f"{name} not in {ASM}"
    return fields


def test_accumulator_bases_not_raised():
    assert open(BASES).read().split() == ["16", "16"]


def test_headline_instance_register_budget():
    md = _metadata(HEADLINE)
    assert int(md["sgpr_spill_count"]) <= SGPR_SPILL_MAX, md["sgpr_spill_count"]
    assert int(md["vgpr_spill_count"]) == 0
    assert int(md["private_segment_fixed_size"]) == 0
