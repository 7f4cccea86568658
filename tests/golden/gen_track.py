"""Writes tests/golden/track_cases.npz: the fixture cases of tests/track_ref.py (CASES) with the restatement's outputs, and one short
undistortedPoints sequence per camera.  Run from anywhere: python tests/golden/gen_track.py

Per case `name`: name/cam (model, cx, cy, c, d, e, poly[5]), cur, forw (float32 [N, 2]), samples (int32 [S, 8]) and the outputs of
track_ref.reject: status, best_sample, num_inliers, mask and, where the device would run (N >= 8), bearing_cur, bearing_forw.  The
essential matrix is not recorded: its last bits are the LAPACK build's, the mask's are not (conditions C1 and C2, which
tests/test_track_ref.py asserts for every case with a model).
Per sequence `seq_k`: seq_k/cam, seq_k/calls and per call j: seq_k/j/pts, ids, time and the outputs un_pts, un_pts_3d, velocity_3d,
matched of track_ref.Undistort."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "track_cases.npz")
SEQUENCES = (("seq_pal", "PAL", 21), ("seq_skew", "SKEW", 22))


def build():
    import track_ref as tr

    out = {"names": np.array(list(tr.CASES))}
    for name in tr.CASES:
        cam, cur, forw, samples = tr.make_case(name)
        r = tr.reject(cam, cur, forw, samples)
        out.update({f"{name}/cam": tr.cam_vector(cam), f"{name}/cur": cur, f"{name}/forw": forw, f"{name}/samples": samples,
                    f"{name}/status": np.int32(r["status"]), f"{name}/best_sample": np.int32(r["best_sample"]),
                    f"{name}/num_inliers": np.int32(r["num_inliers"]), f"{name}/mask": r["mask"]})
        if r["status"] != 2:
            out.update({f"{name}/bearing_cur": r["bearing_cur"], f"{name}/bearing_forw": r["bearing_forw"]})
    out["sequences"] = np.array([s[0] for s in SEQUENCES])
    for name, cam_name, seed in SEQUENCES:
        cam = getattr(tr, cam_name)
        seq, state = tr.undistort_sequence(seed, cam), tr.Undistort()
        out[f"{name}/cam"], out[f"{name}/calls"] = tr.cam_vector(cam), np.int32(len(seq))
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
