"""Writes tests/golden/camera_cases.npz: the fixture cases of tests/camera_ref.py (CASES) with the restatement's outputs, and one short
undistortedPoints sequence per camera.  Run from anywhere: python tests/golden/gen_camera.py

Per case `name`: name/cam (camera_ref.KEYS: model, cx, cy, fx, fy, k1, k2, p1, p2, xi), cur, forw (float32 [N, 2]), samples (int32
[S, 8]) and the outputs of camera_ref.reject: status, best_sample, num_inliers, mask and, where the device would run (N >= 8),
bearing_cur, bearing_forw.  The essential matrix is not recorded, as in track_cases.npz (gen_track.py).
Per sequence `seq_k`: seq_k/cam, seq_k/calls and per call j: seq_k/j/pts, ids, time and the outputs un_pts, un_pts_3d, velocity_3d,
matched of camera_ref.Undistort."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "camera_cases.npz")
SEQUENCES = (("seq_euroc", "EUROC", 21), ("seq_mv3dm", "MV3DM", 22), ("seq_euroc_nd", "EUROC_ND", 23), ("seq_mv3dm_nd", "MV3DM_ND", 24),
             ("seq_mei_xi1", "MEI_XI1", 25))


def build():
    import camera_ref as cr

    out = {"names": np.array(list(cr.CASES))}
    for name in cr.CASES:
        cam, cur, forw, samples = cr.make_case(name)
        r = cr.reject(cam, cur, forw, samples)
        out.update({f"{name}/cam": cr.cam_vector(cam), f"{name}/cur": cur, f"{name}/forw": forw, f"{name}/samples": samples,
                    f"{name}/status": np.int32(r["status"]), f"{name}/best_sample": np.int32(r["best_sample"]),
                    f"{name}/num_inliers": np.int32(r["num_inliers"]), f"{name}/mask": r["mask"]})
        if r["status"] != 2:
            out.update({f"{name}/bearing_cur": r["bearing_cur"], f"{name}/bearing_forw": r["bearing_forw"]})
    out["sequences"] = np.array([s[0] for s in SEQUENCES])
    for name, cam_name, seed in SEQUENCES:
        cam = cr.CAMERAS[cam_name]
        seq, state = cr.undistort_sequence(seed, cam), cr.Undistort()
        out[f"{name}/cam"], out[f"{name}/calls"] = cr.cam_vector(cam), np.int32(len(seq))
        for j, (pts, ids, time) in enumerate(seq):
            r = state(cam, pts, ids, time)
            out.update({f"{name}/{j}/pts": pts, f"{name}/{j}/ids": ids, f"{name}/{j}/time": np.float64(time)})
            out.update({f"{name}/{j}/{k}": v for k, v in r.items()})
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lf-vio_amd"))
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
