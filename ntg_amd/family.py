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


def module_command(source: str, out: str, abi: str | None = None) -> list[str]:
    """hipcc command line of one module (abi: another header stamp than this tree's -- tests of the refusal only)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", os.path.abspath(source), "-o", out,
            "-I", os.path.join(_b.HERE, "..", "include"), "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
            "-DNTG_AMD_ABI=" + (abi or _b.abi_stamp()), "-shared", "-fvisibility=hidden", "-Wl,--no-undefined",
            "-Wl,--version-script=" + os.path.join(_b.CSRC, "family_module.map"),   # kernel handles of template instances escape -fvisibility
            "-save-temps=obj", "-Wno-unused-command-line-argument"] + os.environ.get("NTG_AMD_CXXFLAGS", "").split()


def assembly_path(source: str, out: str | None = None) -> str:
    """device assembly hipcc -save-temps=obj kept for a module: named after the source, next to the output"""
    out = out or module_path(source)
    return os.path.join(os.path.dirname(os.path.abspath(out)), os.path.splitext(os.path.basename(source))[0] + _ASM_SUFFIX)


def finish_module(source: str, out: str) -> str:
    """after hipcc: audit the device assembly, drop the other -save-temps files; on a violation the .so is removed"""
    from . import call_audit
    stem = os.path.splitext(os.path.basename(source))[0]
    d = os.path.dirname(os.path.abspath(out))
    asm = assembly_path(source, out)
    for f in os.listdir(d):
        if (f.startswith(stem + "-hip-") or f.startswith(stem + "-host-") or f.startswith(stem + ".hip-")) and not f.endswith("gfx950.s"):
            os.remove(os.path.join(d, f))
    bad = call_audit.audit(asm) if os.path.exists(asm) else ["no device assembly at " + asm]
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
    r = subprocess.run(module_command(source, out, abi), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("hipcc failed for family module %s:\n%s" % (source, r.stdout[-4000:]))
    return finish_module(source, out)
