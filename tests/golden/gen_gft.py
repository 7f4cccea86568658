"""Writes tests/golden/gft_cases.npz: for every case below what the numpy restatement gft_ref.gft returns — kept indices, corners,
[num_candidates], max_response — and, for the case with tracked points, the points and counts.  The images are not stored:
gft_ref renders them from the seed.  Run from the repository root: python tests/golden/gen_gft.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gft_ref as g  # noqa: E402

TEXTURES = ((345, 339), (161, 123), (97, 75))  # seed 0
DISTANCES = (30, 10, 5, 1, 0)
COUNTS = (150, 4096)
NOISE = (640, 480, 0, 1, 500)  # width, height, seed, min_distance, max_count
TILED = (100, 84, 0, 3, 4096)
MASKED = dict(size=(345, 339), annulus=(172, 169, 160, 20), max_count=150, min_distance=30, mask_radius=30)


def images():
    out = {f"tex_{w}x{h}": g.textured(w, h, 0) for w, h in TEXTURES}
    out["noise"] = g.noise(*NOISE[:3])
    out["tiled"] = g.tiled(*TILED[:3])
    out["truth"] = g.truth_image()
    return out


def masked_inputs():
    w, h = MASKED["size"]
    pts, cnt = g.tracked_case(w, h, 0)
    return g.annulus_mask(w, h, *MASKED["annulus"]), pts, cnt


def build():
    out = {}
    img = images()
    lam = {key: g.response(v) for key, v in img.items()}

    def put(key, r):
        out[key + "_kept"] = r["kept"]
        out[key + "_corners"] = r["corners"]
        out[key + "_counts"] = np.array([r["num_candidates"]], np.int32)
        out[key + "_max"] = np.array([r["max_response"]], np.float64)

    for w, h in TEXTURES:
        name = f"tex_{w}x{h}"
        for d in DISTANCES:
            for mc in COUNTS:
                put(f"{name}_d{d}_m{mc}", g.gft(img[name], max_count=mc, min_distance=d, lam=lam[name]))
    put("noise", g.gft(img["noise"], max_count=NOISE[4], min_distance=NOISE[3], lam=lam["noise"]))
    put("tiled", g.gft(img["tiled"], max_count=TILED[4], min_distance=TILED[3], lam=lam["tiled"]))
    put("truth", g.gft(img["truth"], max_count=150, min_distance=5, lam=lam["truth"]))
    base, pts, cnt = masked_inputs()
    name = "tex_%dx%d" % MASKED["size"]
    out["masked_pts"], out["masked_cnt"] = pts, cnt
    put("masked", g.gft(img[name], base, pts, cnt, max_count=MASKED["max_count"], min_distance=MASKED["min_distance"], mask_radius=MASKED["mask_radius"], lam=lam[name]))
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "gft_cases.npz"), **build())
