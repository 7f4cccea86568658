"""Recordings with raw images on the device: the C++ FeatureTracker (host/feature_tracker.cpp, through lfvio_host_track_trace) against
node_ref.ImageNode, and pixels to poses (lfvio_host_replay_images) against replay() of the pre-tracked recording.

  1  the 161 x 123 sequence of tests/test_tracker_chain.py, its six frames walked back and forth, with a 10 Hz stretch, a 30 Hz
     stretch (some frames are tracked only), a gap of more than a second and a stamp that goes backwards: every message and every
     restart the C++ tracker emits equals the restatement's, bit for bit, and every other record is copied
  2  a make_image_stream recording: replay_images(in) writes the trajectory of replay(track_trace(in)), byte for byte, with equal
     stats; one bootstrap, no failure, a pose for every published message from the eleventh on, 30 rows or more from the third on"""
import os
import sys

import numpy as np
import pytest

import node_ref as nr
from test_tracker_chain import CAM, MAX_CNT, MIN_DIST, frames, same

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))  # ate

pytestmark = pytest.mark.gpu

SEED = 20240611


def stamps_and_frames():
    imgs = frames()
    walk = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]
    t, out = 20.0, []
    plan = [(0.1, 8), (1.0 / 30.0, 12), (0.1, 3), (1.5, 1), (0.1, 4), (-0.25, 1), (0.1, 4)]  # (step, images)
    k = 0
    for dt, n in plan:
        for _ in range(n):
            t += dt
            out.append((t, imgs[walk[k % len(walk)]]))
            k += 1
    return out


def test_cpp_tracker_equals_the_restatement(eng, tmp_path):
    """Test 1."""
    from lfvio import trace
    from lfvio.host import HostEstimator

    seq = stamps_and_frames()
    src, dst = str(tmp_path / "raw.lfvt"), str(tmp_path / "tracked.lfvt")
    w = trace.TraceWriter(src)
    for k, (t, img) in enumerate(seq):
        w.imu(t - 0.01, [0.0, 0.0, 9.8], [0.0, 0.0, 0.0])
        w.image(t, img, step=None if k % 3 else 176)  # every third image with padded rows
        if k % 5 == 0:
            w.truth(t, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0])
    w.close()
    # the restatement
    eng.clahe_set(None)
    eng.gft_set_mask(None)
    node = nr.ImageNode(eng, CAM, max_cnt=MAX_CNT, min_dist=MIN_DIST, freq=10, num_samples=100, seed=SEED)
    want = [(t,) + node.on_image(t, img) for t, img in seq]
    kinds = [x[1] for x in want]
    assert kinds[0] == nr.DROP and kinds.count(nr.RESTART) == 2 and kinds.count(nr.FIRST_PUBLICATION) == 1
    assert kinds.count(nr.TRACKED) >= 4 and kinds.count(nr.PUBLISHED) >= 12 and kinds.count(nr.DROP) == 3
    # the C++ tracker
    he = HostEstimator()
    try:
        he.track_config(CAM, max_cnt=MAX_CNT, min_dist=MIN_DIST, freq=10, num_samples=100, seed=SEED)
        rc, ts = he.track_trace(src, dst)
    finally:
        he.close()
    assert rc == 0, rc
    got = trace.read_trace(dst)
    msgs = [(t, rows) for t, what, rows in want if what == nr.PUBLISHED]
    assert len(got["images"]) == len(msgs)
    for k, ((t, rows), (gt, grows)) in enumerate(zip(msgs, got["images"])):
        assert gt == t and same(grows, rows), k
    assert sum(len(r) for _, r in msgs) > 200 and all(len(r) >= 10 for _, r in msgs[2:])
    assert got["restart_stamps"] == [t for t, what, _ in want if what == nr.RESTART]
    # the order of the records: every image replaced by a message, a restart or nothing, the rest copied
    order = []
    for k, (t, what, _) in enumerate(want):
        order.append(trace.REC_IMU)
        order += {nr.PUBLISHED: [trace.REC_FEATURES], nr.RESTART: [trace.REC_RESTART]}.get(what, [])
        if k % 5 == 0:
            order.append(trace.REC_TRUTH)
    assert got["order"] == order
    raw = trace.read_trace(src)
    assert np.array_equal(got["imu"], raw["imu"]) and np.array_equal(got["truth"], raw["truth"]) and not got["raw_images"]
    assert ts == dict(raw_images=len(seq), dropped=kinds.count(nr.DROP), restarts=2,
                      tracked_only=kinds.count(nr.TRACKED) + 1, published=len(msgs), rows=sum(len(r) for _, r in msgs), tracker_ms=ts["tracker_ms"])
    assert ts["tracker_ms"] > 0.0


def test_pixels_to_poses(tmp_path):
    """Test 2.  Scale 4 (320 x 240), 10 Hz, 36 images, MAX_CNT 80, MIN_DIST 12, S = 100.  The conditions were met by the restatement
    alone on the CPU before this test was written: tests/track_frame_ref.py under node_ref.Gate for the frames
    (34 messages of 63 .. 80 rows), the host sources over the CPU checker for the replay of the derived recording (one bootstrap,
    no failure, 24 poses).  The ATE is printed, not judged: its size is a property of the scene."""
    import ate
    from lfvio import trace
    from lfvio.host import HostEstimator

    src, mid = str(tmp_path / "images.lfvt"), str(tmp_path / "tracked.lfvt")
    j1, j2 = str(tmp_path / "direct.txt"), str(tmp_path / "two_steps.txt")
    made = trace.make_image_stream(src, seed=0, n_frames=36, scale=4)
    out = []
    for direct in (True, False):
        he = HostEstimator()  # a fresh estimator and context for either route
        try:
            he.clear_state()
            he.set_min_parallax(10.0)
            he.set_solver_time(0.0)  # (no wall-clock cap: the number of iterations must not depend on the clock)
            he.track_config(made["camera"], max_cnt=80, min_dist=12, freq=10, num_samples=100, seed=77, annulus=made["annulus"])
            if direct:
                rc, st, ts = he.replay_images(src, j1)
            else:
                rc0, ts = he.track_trace(src, mid)
                assert rc0 == 0
                rc, st = he.replay(mid, j2)
            out.append((rc, st, {k: v for k, v in ts.items() if k != "tracker_ms"}))
        finally:
            he.close()
    assert out[0] == out[1], out
    rc, st, ts = out[0]
    a, b = open(j1, "rb").read(), open(j2, "rb").read()
    assert a == b and len(a) > 0
    assert rc == 0 and st["bootstraps"] == 1 and st["failures"] == 0 and st["last_status"] == 0, st
    tracked = trace.read_trace(mid)
    msgs = tracked["images"]
    assert ts["published"] == len(msgs) == 34 and ts["dropped"] == 1 and ts["tracked_only"] == 1 and ts["restarts"] == 0 and ts["raw_images"] == 36
    assert [t for t, _ in msgs] == made["stamps"][2:]
    # a pose for every published message from the eleventh on (the last image waits for an IMU sample behind it, as in every replay)
    assert st["images"] in (len(msgs) - 1, len(msgs)) and st["poses"] == st["images"] - 10, st
    assert all(len(rows) >= 30 for _, rows in msgs[2:]), [len(rows) for _, rows in msgs]
    lines = a.decode().strip().split("\n")
    assert len(lines) == st["poses"]  # (the file holds twelve decimals of a stamp)
    assert np.allclose([float(ln.split(" ")[0]) for ln in lines], [t for t, _ in msgs[10:10 + st["poses"]]], rtol=0, atol=1e-9)
    print("pixels to poses: ATE", ate.ate(j1, src), "rows", [len(rows) for _, rows in msgs], "stats", st)
