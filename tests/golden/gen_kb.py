"""Writes tests/golden/kb_cases.npz: the fixture cases of tests/kb_ref.py (CASES) with the restatement's outputs, and one short
undistortedPoints sequence per camera, in the layout of camera_cases.npz (gen_camera.py).  Run from anywhere:
python tests/golden/gen_kb.py

Per case `name`: name/cam (kb_ref.KEYS: model, cx, cy, fx, fy, k2, k3, k4, k5), cur, forw (float32 [N, 2]), samples (int32 [S, 8]) and
the outputs of kb_ref.reject: status, best_sample, num_inliers, mask and, where the device would run (N >= 8), bearing_cur,
bearing_forw.
Per sequence `seq_k`: seq_k/cam, seq_k/calls and per call j: seq_k/j/pts, ids, time and the outputs un_pts, un_pts_3d, velocity_3d,
matched of kb_ref.Undistort."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kb_cases.npz")
SEQUENCES = (("seq_tum", "TUM", 21), ("seq_cla", "CLA", 22), ("seq_rsfish", "RSFISH", 23), ("seq_kb_k5_0", "KB_K5_0", 24),
             ("seq_kb_k45_0", "KB_K45_0", 25), ("seq_kb_ideal", "KB_IDEAL", 26))


def build():
    import kb_ref as kb

    out = {"names": np.array(list(kb.CASES))}
    for name in kb.CASES:
        cam, cur, forw, samples = kb.make_case(name)
        r = kb.reject(cam, cur, forw, samples)
        out.update({f"{name}/cam": kb.cam_vector(cam), f"{name}/cur": cur, f"{name}/forw": forw, f"{name}/samples": samples,
                    f"{name}/status": np.int32(r["status"]), f"{name}/best_sample": np.int32(r["best_sample"]),
                    f"{name}/num_inliers": np.int32(r["num_inliers"]), f"{name}/mask": r["mask"]})
        if r["status"] != 2:
            out.update({f"{name}/bearing_cur": r["bearing_cur"], f"{name}/bearing_forw": r["bearing_forw"]})
    out["sequences"] = np.array([s[0] for s in SEQUENCES])
    for name, cam_name, seed in SEQUENCES:
        cam = kb.CAMERAS[cam_name]
        seq, state = kb.undistort_sequence(seed, cam, size=kb.SIZES[cam_name]), kb.Undistort()
        out[f"{name}/cam"], out[f"{name}/calls"] = kb.cam_vector(cam), np.int32(len(seq))
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
