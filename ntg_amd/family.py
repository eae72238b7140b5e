"""Build a user problem family into a loadable module (include/ntg_amd_family.hpp, INTEGRATION.md "Your own problem family").

    from ntg_amd import family, api
    so = family.build_module("my_family.hip")     # -> my_family.so next to the source
    fam = api.load_family(so)                     # id for Spec.family

The module is compiled with the library's flags and its header stamp (-DNTG_AMD_ABI, see build.abi_stamp), with hidden visibility
(only the entry point ntg_family_module_v1 is exported: every module instantiates kernels under the same names, and only hidden host
stubs plus dlopen(RTLD_LOCAL) keep their launches apart), and linked with --no-undefined.  Its device assembly is kept and audited
by call_audit before the shared object is handed out: a callback that forces an out-of-line call with a private-segment pointer is
the pattern that once faulted a GPU, and a module refused here never reaches one.
"""
from __future__ import annotations
import os
import re
import subprocess
import sys

from . import build as _b

_ASM_SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def module_path(source: str) -> str:
    return os.path.splitext(os.path.abspath(source))[0] + ".so"


def _local_includes(source: str) -> list[str]:
    """headers the source includes by a quoted path that exists next to it (one level: enough for a family header)"""
    d = os.path.dirname(os.path.abspath(source))
    out = []
    for m in re.finditer(r'^\s*#\s*include\s+"([^"]+)"', open(source).read(), flags=re.M):
        p = os.path.join(d, m.group(1))
        if os.path.exists(p):
            out.append(p)
    return out


def stale(source: str, out: str | None = None) -> bool:
    """the module is missing, or older than its source, a header next to the source it includes, or any of the library's HEADERS"""
    out = out or module_path(source)
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [source] + _local_includes(source) + [os.path.join(_b.CSRC, f) for f in _b.HEADERS + ["family_module.map"]]
    return any(os.path.getmtime(f) > t for f in deps if os.path.exists(f))


def _check_unit(source: str, out: str) -> tuple[str, str, str]:
    """files of a module's second compilation (its check_kernel and cost_kernel instances, NTG_AMD_MODULE_PART = 2): a one-line wrapper source next to
    the output -- a name of its own, so that hipcc -save-temps keeps its device assembly apart -- its object, and the first part's object"""
    stem = os.path.splitext(os.path.basename(source))[0]
    d = os.path.dirname(os.path.abspath(out))
    return os.path.join(d, stem + "_check.hipx"), os.path.join(d, stem + "_check.o"), os.path.join(d, stem + ".o")


def write_check_unit(source: str, out: str) -> None:
    """the wrapper source of the second compilation (removed again by finish_module / build_module)"""
    with open(_check_unit(source, out)[0], "w") as f:
        f.write('#include "%s"\n' % os.path.abspath(source))


def module_commands(source: str, out: str, abi: str | None = None) -> tuple[list[str], list[str], list[str]]:
    """hipcc command lines of one module (abi: another header stamp than this tree's -- tests of the refusal only): the two
    compilations of the source, independent of each other -- everything but the check and cost instances (part 1), those two from the
    wrapper of write_check_unit (part 2) -- and the link of their objects"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    wrap, cobj, mobj = _check_unit(source, out)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(_b.HERE, "..", "include"), "-Wno-unused-result",
             "-Wno-unused-value", "-Wno-pass-failed", "-DNTG_AMD_ABI=" + (abi or _b.abi_stamp()), "-fvisibility=hidden", "-save-temps=obj",
             "-Wno-unused-command-line-argument"] + os.environ.get("NTG_AMD_CXXFLAGS", "").split()
    part1 = [hipcc] + flags + ["-DNTG_AMD_MODULE_PART=1", "-x", "hip", "-c", os.path.abspath(source), "-o", mobj]
    part2 = [hipcc] + flags + ["-DNTG_AMD_MODULE_PART=2", "-x", "hip", "-c", wrap, "-o", cobj]
    link = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", mobj, cobj, "-o", out, "-Wl,--no-undefined",
            "-Wl,--version-script=" + os.path.join(_b.CSRC, "family_module.map")]   # kernel handles of template instances escape -fvisibility
    return part1, part2, link


def assembly_path(source: str, out: str | None = None) -> str:
    """device assembly hipcc -save-temps=obj kept for a module's evaluation and solve instances: named after the source, next to the output"""
    out = out or module_path(source)
    return os.path.join(os.path.dirname(os.path.abspath(out)), os.path.splitext(os.path.basename(source))[0] + _ASM_SUFFIX)


def check_assembly_path(source: str, out: str | None = None) -> str:
    """... and for its check instance (the second compilation)"""
    out = out or module_path(source)
    return os.path.splitext(_check_unit(source, out)[0])[0] + _ASM_SUFFIX


def remove_check_unit(source: str, out: str) -> None:
    for f in _check_unit(source, out):
        if os.path.exists(f):
            os.remove(f)


def finish_module(source: str, out: str) -> str:
    """after hipcc: audit the device assembly of both compilations, drop the other -save-temps files; on a violation the .so is removed"""
    from . import call_audit
    stem = os.path.splitext(os.path.basename(source))[0]
    d = os.path.dirname(os.path.abspath(out))
    for f in os.listdir(d):
        for st in (stem, stem + "_check"):
            if (f.startswith(st + "-hip-") or f.startswith(st + "-host-") or f.startswith(st + ".hip-") or f.startswith(st + ".hipx-")) and not f.endswith("gfx950.s"):
                os.remove(os.path.join(d, f))
    remove_check_unit(source, out)
    bad = []
    for asm in (assembly_path(source, out), check_assembly_path(source, out)):
        bad += call_audit.audit(asm) if os.path.exists(asm) else ["no device assembly at " + asm]
    if bad:
        os.remove(out)
        raise RuntimeError("call-boundary audit of family module %s failed:\n  %s" % (source, "\n  ".join(bad[:20])))
    return out


def build_module(source: str, out: str | None = None, abi: str | None = None, force: bool = False) -> str:
    """Compile `source` (a .hip file using NTG_AMD_FAMILY_MODULE) into a module; returns the path of the .so.  Rebuilds only when
    stale (see stale()); `abi` overrides the header stamp (tests of the refusal at load)."""
    out = os.path.abspath(out or module_path(source))
    if not force and abi is None and not stale(source, out):
        return out
    write_check_unit(source, out)
    try:
        for cmd in module_commands(source, out, abi):
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout)
                raise RuntimeError("hipcc failed for family module %s:\n%s" % (source, r.stdout[-4000:]))
        return finish_module(source, out)
    finally:
        remove_check_unit(source, out)
