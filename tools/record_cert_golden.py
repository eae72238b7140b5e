"""Record tests/golden/cert_calls.npz (tests/test_gpu_cert_golden.py) with the library named by NTG_AMD_LIB -- meant for the library of
the commit BEFORE a change to the time certificates (envelope, envelope_sos, extrema) that must not move a bit.

  NTG_AMD_LIB=LIB python tools/record_cert_golden.py [OUT.npz]     on the GPU

The cases are in tests/cert_golden_cases.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    lib = os.environ.get("NTG_AMD_LIB")
    if not lib:
        sys.exit("set NTG_AMD_LIB to the library to record from")
    import numpy as np
    import cert_golden_cases as wc
    from ntg_amd import api
    assert os.path.abspath(api.LIB_PATH) == os.path.abspath(lib)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cert_calls.npz")
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
