"""Writes tests/golden/fuse_cases.npz: a few hundred recorded points of tests/fuse_ref.py with the specification's outputs.
Run from anywhere: python tests/golden/gen_fuse.py

P (float32 [n, 3]): seeded points over the sphere and fuse_ref.special_cloud.  poses: the three of fuse_ref.poses; per pose `p`: p/R,
p/T, and at 33 x 17 EQUIRECT with the gate [0.5, 100] p/index (int32 [n]), p/why (int32 [n]), p/range (float32 [17, 33]).  cams: one
camera of each model; per camera `c`: c/cam (project_ref.cam_vector of the camera scaled to a 64 x 48 image), c/P (float32 [m, 3]) and
c/index, c/why, c/range (float32 [48, 64]) of LFVIO_FUSE_CAMERA through the identity."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fuse_cases.npz")
CAMS = ("PAL", "EUROC", "MV3DM", "TUM")
W, H, CW, CH = 33, 17, 64, 48
GATE = (0.5, 100.0)


def small_cam(name):
    import project_ref as pr

    cam, (cw, _) = pr.CAMS[name]
    return pr.small(cam, cw / CW)


def build():
    import fuse_ref as fr
    import project_ref as pr

    P = np.concatenate([fr.sphere_cloud(200, seed=7), fr.special_cloud()])
    out = {"P": P, "poses": np.array([p[0] for p in fr.poses()]), "cams": np.array(CAMS)}
    for name, R, T in fr.poses():
        v = fr.view(width=W, height=H, R=R, T=T, min_range=GATE[0], max_range=GATE[1])
        index, rf, why = fr.points(v, P[:, 0], P[:, 1], P[:, 2])
        out.update({f"{name}/R": np.asarray(R, np.float64).reshape(9), f"{name}/T": np.asarray(T, np.float64), f"{name}/index": index, f"{name}/why": why,
                    f"{name}/range": fr.range_image(index, rf, W, H)})
    for k, name in enumerate(CAMS):
        cam = small_cam(name)
        Q = np.concatenate([pr.image_rays(name, 100).astype(np.float32), fr.sphere_cloud(60, seed=20 + k, lo=0.5, hi=30.0),
                            fr.special_cloud()])
        v = fr.view(kind=fr.FUSE_CAMERA, width=CW, height=CH, cam=cam)
        index, rf, why = fr.points(v, Q[:, 0], Q[:, 1], Q[:, 2])
        out.update({f"{name}/cam": pr.cam_vector(cam), f"{name}/P": Q, f"{name}/index": index, f"{name}/why": why, f"{name}/range": fr.range_image(index, rf, CW, CH)})
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lf-vio_amd"))
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
