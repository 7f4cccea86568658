"""Writes tests/golden/clahe_cases.npz: for a few of clahe_ref.CASES what the numpy restatement clahe_ref.clahe returns — the
equalized image and the LUTs.  The inputs are not stored: clahe_ref renders them from the seed.  Run from the repository root:
python tests/golden/gen_clahe.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clahe_ref as c  # noqa: E402

STORED = ("divides_64", "neither_97x75", "one_side_96x75", "tiny_tiles_16", "repeated_16x31", "two_valued_97x75", "no_clip_97x75", "tiles_3x5", "tiles_16x16",
          "residuals", "residuals_batch")


def build():
    out = {}
    for name in STORED:
        cl, tiles = c.CASES[name][4:]
        out[name + "_out"], out[name + "_lut"] = c.clahe(c.case_image(name), cl, tiles)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "clahe_cases.npz"), **build())
