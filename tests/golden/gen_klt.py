"""Writes tests/golden/klt_cases.npz: for every case of tests/klt_ref.py (shapes (a)-(e) of DESIGN.md 3k, seeds 0-3) and the status
case the points and what the float64 restatement klt_ref.track returns for them.  The images are not stored: klt_ref.make_case
renders them from the seed.  Run from the repository root: python tests/golden/gen_klt.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import klt_ref as k  # noqa: E402

SEEDS = (0, 1, 2, 3)
FIELDS = ("next", "status", "iterations")


def build():
    out = {}

    def put(key, c, r):
        out[key + "_pts"] = c["pts"]
        for f in FIELDS:
            out[key + "_" + f] = r[f]
        out[key + "_counts"] = np.array([r["levels_used"], r["num_tracked"]], np.int32)

    for name in sorted(k.CASES):
        for seed in SEEDS:
            c = k.make_case(name, seed)
            put(f"{name}_{seed}", c, k.run_case(c))
    c = k.make_status_case()
    put("status_b1", c, k.run_case(c, border=1))
    put("status_bm1", c, k.run_case(c, border=-1))
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "klt_cases.npz"), **build())
