"""Record what the oracles of the bisection calls return on their seeded inputs -- meant for the oracles of the commit BEFORE a change of
their level loop that must not move a result.  CPU only; no library is loaded.

  python tools/record_oracle_levels.py [OUT.npz]

Writes tests/golden/oracle_levels.npz (tests/test_oracle_levels_golden.py); the cases are in tests/oracle_levels_cases.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import oracle_levels_cases as lc
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oracle_levels.npz")
    arrays = {}
    for name in lc.CASES:
        res = lc.run_case(name)
        for k, v in res.items():
            arrays[name + "/" + k] = v
        status = np.concatenate([v.reshape(-1) for k, v in res.items() if k.endswith("/status")])
        print("%-14s %s  status %s" % (name, " ".join(sorted({k.split("/")[0] for k in res})), sorted(set(status.tolist()))), flush=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
