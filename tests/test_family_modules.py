"""User problem families as loadable modules (include/ntg_amd_family.hpp, ntg_amd/family.py, family_registry.cpp): what can be
checked without a GPU -- the build of the in-tree modules, their exports, loading and refusals (no HIP call), the call-boundary
audit of their device code, and that a module's generic kernels are the built-in family's generic kernels (same resources)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = os.path.join(ROOT, "ntg_amd", "modules")
NTG_E_BADARG = -2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from ntg_amd import family
    return {m: family.build_module(os.path.join(MODULES, m + ".hip")) for m in ("unicycle", "testfam_module")}


def _raw_load(path):
    from ntg_amd import api
    fam = C.c_int(-1)
    rc = api.lib().ntg_family_load(os.fsencode(path), C.byref(fam))
    return rc, fam.value, api.lib().ntg_last_error().decode()


@pytest.mark.parametrize("name", ["unicycle", "testfam_module"])
def test_module_exports_only_its_entry_point(built, name):
    so = built[name]
    assert os.path.exists(so)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    names = [ln.split()[-1] for ln in syms if ln.strip()]
    assert "ntg_family_module_v1" in names
    assert not [n for n in names if "kernel" in n or "launch" in n], names


def test_load_and_info(built):
    from ntg_amd import api
    ids = {}
    for name, dm, counts, nout in (("unicycle", 3, (1, 2, 1), 2), ("testfam_module", 3, (1, 2, 1), 0)):
        fam = api.load_family(built[name])
        assert fam >= 64
        info = api.family_info(fam)
        assert info == dict(name=name, maxderiv=dm, nnlic=counts[0], nnltc=counts[1], nnlfc=counts[2], nout=nout)
        # the same file again, also under another spelling of its path: the same id
        assert api.load_family(built[name]) == fam
        assert api.load_family(os.path.join(MODULES, "..", "modules", os.path.basename(built[name]))) == fam
        ids[name] = fam
    assert ids["unicycle"] != ids["testfam_module"]
    with pytest.raises(api.NtgError):
        api.family_info(63)


def test_refuses_module_built_against_other_headers(built, tmp_path):
    from ntg_amd import build, family
    other = "0x0123456789abcdefull"
    so = family.build_module(os.path.join(MODULES, "testfam_module.hip"), out=str(tmp_path / "other_abi.so"), abi=other)
    rc, _, msg = _raw_load(so)
    assert rc == NTG_E_BADARG
    assert "0123456789abcdef" in msg and build.abi_stamp()[2:18] in msg, msg


def test_refuses_shared_object_without_entry_point(built, tmp_path):
    src = tmp_path / "plain.c"
    src.write_text("int not_a_family(void) { return 1; }\n")
    so = tmp_path / "plain.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    rc, _, msg = _raw_load(str(so))
    assert rc == NTG_E_BADARG and "ntg_family_module_v1" in msg, msg


def test_refuses_missing_file(built, tmp_path):
    rc, _, msg = _raw_load(str(tmp_path / "nowhere.so"))
    assert rc == NTG_E_BADARG and "nowhere.so" in msg, msg


@pytest.mark.parametrize("name", ["unicycle", "testfam_module"])
def test_call_audit_passes_on_module_assembly(built, name):
    from ntg_amd import call_audit, family
    asm = family.assembly_path(os.path.join(MODULES, name + ".hip"))
    assert os.path.exists(asm)
    assert call_audit.audit(asm) == []


def _kernel_resources(path):
    """per kernel of a device assembly: the register, LDS and scratch fields of its kernel descriptor"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1); out[cur] = {}
            continue
        if cur and ".end_amdhsa_kernel" in line:
            cur = None
            continue
        if cur:
            m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)", line)
            if m:
                out[cur][m.group(1)] = m.group(2)
    return out


def test_restated_testfam_compiles_to_the_builtin_generic_kernels(built):
    """the module's generic sqp_kernel / eval_kernel instances use exactly the VGPR, SGPR, LDS and scratch of fam_testfam's generic
    instances: the same code (only the family slot in the kernel name differs)"""
    from ntg_amd import family
    mod = _kernel_resources(family.assembly_path(os.path.join(MODULES, "testfam_module.hip")))
    lib = _kernel_resources(os.path.join(ROOT, "ntg_amd", "csrc", "fam_testfam-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert len(mod) == 8   # eval at 128 / 256 / 512 threads, sqp at 128 / 256 / 512 plus BIG at 256 / 512
    for name, res in mod.items():
        twin = name.replace("ILi1000E", "ILi2E", 1)
        assert twin in lib, twin
        assert len(res) == 5 and res == lib[twin], (name, res, lib[twin])
