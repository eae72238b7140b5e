"""Record tests/golden/wave_instances.npz (tests/test_gpu_wave_golden_instances.py), with --restarts tests/golden/wave_restarts.npz
(tests/test_gpu_wave_golden_restarts.py), with --tail tests/golden/wave_tail.npz (tests/test_gpu_wave_golden_tail.py), with --exits
tests/golden/wave_exits.npz (solves that end at the iteration limit: tests/test_gpu_wave_golden_exits.py), with --norms
tests/golden/wave_norms.npz (solves through the consumers of the iterate's norms and of |g|^2: tests/test_gpu_wave_golden_norms.py) or with --sqp
tests/golden/sqp_modes.npz (the Newton and QP modes of sqp_kernel: tests/test_gpu_sqp_golden.py) with the library named by NTG_AMD_LIB --
meant for the library of the commit BEFORE a change that must not move a bit.

  python tools/record_wave_golden.py --audit LIB     where LIB was built (no GPU): audit the device assembly of its wave kernels
                                                     (ntg_amd/isa_audit.py) and the call boundaries of every unit's (ntg_amd/call_audit.py),
                                                     and write LIB.audited
  NTG_AMD_LIB=LIB python tools/record_wave_golden.py [--restarts | --tail | --exits | --norms | --sqp] [OUT.npz]     on the GPU: refuses a library without a matching LIB.audited

A library whose wave kernels failed the audit may corrupt the chain or fault on the GPU: it is never run."""
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _assembly_of(lib):
    """the wave unit's device assembly next to a library: ntg_amd/build.py keeps it under csrc/, tools/mkvariant.sh as wave_NAME.s"""
    d, base = os.path.dirname(lib), os.path.basename(lib)
    cands = [os.path.join(d, "csrc", "fam_kincar_wave-hip-amdgcn-amd-amdhsa-gfx950.s")]
    if base.startswith("libntg_") and base.endswith(".so"):
        cands.append(os.path.join(d, "wave_" + base[len("libntg_"):-3] + ".s"))
    for c in cands:
        if os.path.exists(c) and os.path.getmtime(c) <= os.path.getmtime(lib):
            return c
    return None


def audit(lib):
    from ntg_amd import call_audit, isa_audit
    asm = _assembly_of(lib)
    if asm is None:
        sys.exit("no device assembly of the wave kernels next to %s (or newer than it): nothing to audit" % lib)
    bad = isa_audit.audit("hipcc", "", "", [], 16, asm_path=asm)
    for a in sorted(glob.glob(os.path.join(os.path.dirname(asm), "*-gfx950.s")) if asm.endswith("-gfx950.s") else [asm]):   # (the --sqp cases run the other units' kernels)
        bad += call_audit.audit(a)
    if bad:
        sys.exit("audit FAILED for %s:\n  %s" % (lib, "\n  ".join(b[:200] for b in bad[:8])))
    with open(lib + ".audited", "w") as f:
        f.write(_sha(lib) + "\n")
    print("audit passed:", asm, "->", lib + ".audited")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--audit":
        return audit(os.path.abspath(sys.argv[2]))
    lib = os.environ.get("NTG_AMD_LIB")
    if not lib:
        sys.exit("set NTG_AMD_LIB to the library to record from")
    lib = os.path.abspath(lib)
    try:
        ok = open(lib + ".audited").read().split()[0] == _sha(lib)
    except OSError:
        ok = False
    if not ok:
        sys.exit("%s has no matching .audited stamp (run --audit where it was built): not run" % lib)
    import numpy as np
    args = [a for a in sys.argv[1:] if a not in ("--restarts", "--tail", "--exits", "--norms", "--sqp")]
    if "--sqp" in sys.argv[1:]:
        import sqp_golden_cases as wc
        default = "sqp_modes.npz"
    elif "--norms" in sys.argv[1:]:
        import wave_golden_norms_cases as wc
        default = "wave_norms.npz"
    elif "--exits" in sys.argv[1:]:
        import wave_golden_exit_cases as wc
        default = "wave_exits.npz"
    elif "--tail" in sys.argv[1:]:
        import wave_golden_tail_cases as wc
        default = "wave_tail.npz"
    elif "--restarts" in sys.argv[1:]:
        import wave_golden_restart_cases as wc
        default = "wave_restarts.npz"
    else:
        import wave_golden_cases as wc
        default = "wave_instances.npz"
    from ntg_amd import api
    assert os.path.abspath(api.LIB_PATH) == lib
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", default)
    arrays = {}
    for name in wc.CASES:
        res = wc.run_case(name)
        if isinstance(res, tuple):   # (--sqp: with the kernel the plan names for the solve)
            res, arrays[name + "/kernel"] = res[0], np.array(res[1])
        for k in (wc.keys_of(name) if hasattr(wc, "keys_of") else wc.KEYS):   # (--exits: clambda too where the case asks for it)
            arrays[name + "/" + k] = res[k]
        print("%-20s iters %s nfev %s inform %s" % (name, res["iters"].tolist(), res["nfev"].tolist(), res["inform"].tolist()), flush=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
