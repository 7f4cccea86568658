"""One image after the other through lfvio.tracker.FeatureTracker — readImage as device calls only — checked stage by stage on the
inputs the device stage actually had:

  reject     equals lfvio_two_view on the restatement's bearings of the same matches and sample sets (tests/test_track.py, test 2)
  detect     equals gft_ref.gft bit for bit
  undistort  equals track_ref.Undistort bit for bit
  (the flow is tests/test_klt.py's business and is not judged again)

and the invariants of the chain: ids are unique, a survivor's count grows by one per frame, a corner's velocity is zero on its first
two frames (it enters the map under -1: the reference's quirk) and non-zero from the third.

Six frames of a klt_ref-rendered 161 x 123 sequence, MAX_CNT 40, MIN_DIST 10; the camera is the PAL camera scaled to the image."""
import numpy as np
import pytest

import gft_ref
import klt_ref
import track_ref as tr
from lfvio import synth

pytestmark = pytest.mark.gpu

W, H, FRAMES, MAX_CNT, MIN_DIST, SCALE = 161, 123, 6, 40, 10, 8.0
# the PAL polynomial in pixels of an image 8 times smaller: z' (phi') = z (8 phi') / 8
CAM = dict(cx=80.25, cy=61.5, c=1.0, d=0.0, e=0.0, poly=tuple(c * SCALE ** i / SCALE for i, c in enumerate(synth.OCAM_POLY)))


def frames():
    f = klt_ref.texture(5)
    out = []
    for k in range(FRAMES):
        _, inv = klt_ref.warp(W, H, shift=(1.5 * k, -0.75 * k), scale=0.004 * k, angle=0.006 * k)
        out.append(klt_ref.render(f, W, H, inv))
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_six_frames_stage_by_stage(eng):
    from lfvio.tracker import FeatureTracker

    eng.clahe_set(None)
    eng.gft_set_mask(None)
    trk = FeatureTracker(eng, CAM, max_cnt=MAX_CNT, min_dist=MIN_DIST, num_samples=100, seed=3)
    imgs = frames()
    recs = [trk.read_image(img, 20.0 + 0.05 * k) for k, img in enumerate(imgs)]
    state, first_seen, models = tr.Undistort(), {}, 0
    for k, (img, rec) in enumerate(zip(imgs, recs)):
        # reject
        rj = rec["reject"]
        d, N = rj["out"], len(rj["cur"])
        if N < 8:
            assert d["status"] == 2 and np.all(d["mask"] == 1), k
        else:
            t = eng.two_view(tr.bearings(CAM, rj["cur"]), tr.bearings(CAM, rj["forw"]), rj["samples"])
            assert (d["status"], d["best_sample"], d["num_inliers"], d["best_score"]) == (t["status"], t["best_sample"], t["num_inliers"], t["best_score"]), k
            if t["status"] == 0:
                assert same(d["mask"], t["mask"]) and same(d["E"], np.asarray(t["E"], np.float64).reshape(9)), k
                models += 1
            else:
                assert np.all(d["mask"] == 1), k
        # detect
        dt = rec["detect"]
        g = gft_ref.gft(img, pts=dt["pts"], cnt=dt["track_cnt"], max_count=MAX_CNT, quality=0.01, min_distance=MIN_DIST, mask_radius=MIN_DIST)
        assert same(dt["kept"], np.asarray(g["kept"], np.int32)) and same(dt["corners"], np.asarray(g["corners"], np.float32)), k
        # undistort
        un = rec["undistort"]
        r = state(CAM, un["pts"], un["ids"], un["time"])
        for key in ("un_pts", "un_pts_3d", "velocity_3d", "matched"):
            assert same(un["out"][key], r[key]), (k, key)
        # the chain's invariants
        ids, cnt = rec["ids"], rec["track_cnt"]
        assert len(set(ids.tolist())) == len(ids) and np.all(ids >= 0) and len(ids) <= MAX_CNT, k
        for i, c, v in zip(ids.tolist(), cnt.tolist(), rec["velocity_3d"]):
            first_seen.setdefault(i, k)
            age = k - first_seen[i]
            assert c == age + 1, (k, i, c)  # a survivor's count grows by one per frame
            assert v.any() == (age >= 2), (k, i, age, v)
    assert len(recs[0]["ids"]) >= 20 and models >= 3
    assert sum(1 for i, f in first_seen.items() if f == 0 and i in set(recs[-1]["ids"].tolist())) >= 10  # tracks that live all six frames
    assert any(f > 0 for f in first_seen.values())  # and corners that arrived later
