"""Writes tests/golden/remap_cases.npz: the projections and the small maps of tests/project_ref.py with the specification's outputs.
Run from anywhere: python tests/golden/gen_remap.py

names: the 13 cameras.  Per camera `name`: name/cam (project_ref.cam_vector: LfvioCamera's 18 fields and the 20 of inv_poly), name/P
(float64 [66, 3]: rays inside the image, rays over the sphere, the special rays) and name/px = project_ref.project (float64 [66, 2]).
maps: the cases of project_ref.MAPS.  Per map `m`: m/cam, m/kind, m/size (width, height), m/M (zeros for EQUIRECT), m/x, m/y (float32
[height, width]) and, for each (encoding, step) of project_ref.GATHERS, m/out_e_s = project_ref.remap of src_e_s (uint8 [height, width *
bytes per pixel]).  src_e_s (uint8 [48, step]): seeded noise, 64 x 48 pixels, one image per (encoding, step), shared by the maps."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "remap_cases.npz")


def build():
    import project_ref as pr

    out = {"names": np.array(list(pr.CAMS)), "maps": np.array(list(pr.MAPS))}
    for name, (cam, _) in pr.CAMS.items():
        P = pr.fixture_rays(name)
        out.update({f"{name}/cam": pr.cam_vector(cam), f"{name}/P": P, f"{name}/px": pr.project(cam, P)})
    for enc, step in pr.GATHERS:
        out[f"src_{enc}_{step}"] = pr.noise_image(enc + step, pr.SRC_W, pr.SRC_H, enc, step)
    for m in pr.MAPS:
        cam, kind, W, H, M = pr.map_case(m)
        mx, my = pr.build(cam, kind, W, H, M)
        out.update({f"{m}/cam": pr.cam_vector(cam), f"{m}/kind": np.int32(kind), f"{m}/size": np.array([W, H], np.int32),
                    f"{m}/M": np.zeros(9) if M is None else np.asarray(M, np.float64).reshape(9), f"{m}/x": mx, f"{m}/y": my})
        for enc, step in pr.GATHERS:
            out[f"{m}/out_{enc}_{step}"] = pr.remap(out[f"src_{enc}_{step}"], mx, my, pr.SRC_W, pr.SRC_H, enc, step)
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lf-vio_amd"))
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
