"""Record a bitwise fixture of the time certificates with the library named by NTG_AMD_LIB -- meant for the library of the commit BEFORE a
change that must not move a bit.

  NTG_AMD_LIB=LIB python tools/record_cert_golden.py [cert|bisect|interp] [OUT.npz]     on the GPU

  cert     tests/golden/cert_calls.npz (tests/test_gpu_cert_golden.py): envelope, envelope_sos, extrema; cases in tests/cert_golden_cases.py
  bisect   tests/golden/bisect_calls.npz (tests/test_gpu_bisect_golden.py): separation, forms, ratios; cases in tests/bisect_golden_cases.py
  interp   tests/golden/interp_calls.npz (tests/test_gpu_interp_golden.py): Plan.interp, inputs and flags; cases in tests/interp_golden_cases.py"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SETS = {"cert": ("cert_golden_cases", "cert_calls.npz"), "bisect": ("bisect_golden_cases", "bisect_calls.npz"),
        "interp": ("interp_golden_cases", "interp_calls.npz")}


def main():
    lib = os.environ.get("NTG_AMD_LIB")
    if not lib:
        sys.exit("set NTG_AMD_LIB to the library to record from")
    args = sys.argv[1:]
    which = args.pop(0) if args and args[0] in SETS else "cert"
    import numpy as np
    wc = importlib.import_module(SETS[which][0])
    from ntg_amd import api
    assert os.path.abspath(api.LIB_PATH) == os.path.abspath(lib)
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", SETS[which][1])
    arrays = {}
    for name in wc.CASES:
        res = wc.run_case(name)
        for k, v in res.items():
            arrays[name + "/" + k] = v
        print("%-8s %s" % (name, " ".join(sorted({k.split("/")[0] + ("!" if k.endswith("/error") else "") for k in res}))), flush=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
