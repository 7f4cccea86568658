"""CPU tests of recordings with raw images (record type 10 of lf-vio_amd/host/replay.h) and of the message rows' restatement.

  1  TraceWriter.image -> read_trace -> the host loader, an image with step > width among them
  2  every malformed image record is refused with -3, by the product build and by the suite's CPU build of the same sources
  3  a type-10 file through the existing replay: rc 0 and zero images (raw images are no feature messages)
  4  make_image_stream at a tiny size: record order, stamps, the bootstrap's stamp, no pixel lit outside the annulus
  5  tools/bag_to_lfvt.py --image: a bag of sensor_msgs/Image written by BagWriter becomes the same records
  6  node_ref.rows_from_table on hand-made tables: all counts 1, all counts > 1, 0, 17 and 4096 entries"""
import os
import struct
import sys

import numpy as np
import pytest

import node_ref as nr
from lfvio import abi, rosmsg, synth, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as ge

    ge.build()
    from lfvio.host import HostEstimator

    h = HostEstimator()
    yield h
    h.close()


def picture(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def test_writer_reader_and_host_loader(host, tmp_path):
    p = str(tmp_path / "raw.lfvt")
    imgs = [picture(k, 40, 24) for k in range(3)]
    steps = [None, 48, 41]
    w = trace.TraceWriter(p)
    w.imu(0.5, [0, 0, 9.8], [0, 0, 0])
    for k, (img, st) in enumerate(zip(imgs, steps)):
        w.image(1.0 + 0.1 * k, img, step=st)
        w.truth(1.0 + 0.1 * k, [0, 0, 0], [0, 0, 0, 1])
    w.close()
    t = trace.read_trace(p)
    assert t["order"] == [1, 10, 4, 10, 4, 10, 4] and t["raw_steps"] == [40, 48, 41] and not t["images"]
    for k, (stamp, img) in enumerate(t["raw_images"]):
        assert stamp == 1.0 + 0.1 * k and np.array_equal(img, imgs[k])
    assert host.has_tracker
    n, rows, err = host.trace_raw_images(p)
    assert n == 3 and err == ""
    raw = open(p, "rb").read()
    for k, r in enumerate(rows):
        assert (r[0], r[1], r[2], r[3]) == (1.0 + 0.1 * k, 40, 24, t["raw_steps"][k])
        o, step = int(r[4]), int(r[3])
        got = np.frombuffer(raw, np.uint8, count=24 * step, offset=o).reshape(24, step)
        assert np.array_equal(got[:, :40], imgs[k]) and not got[:, 40:].any()


def image_record(t=1.0, w=32, h=16, step=None, enc=0, nbytes=None, says=None):
    """A type-10 record with every field free: nbytes of pixels, `says` in the record's length field."""
    step = w if step is None else step
    nbytes = h * step if nbytes is None else nbytes
    body = struct.pack("<dIIII", t, w, h, step, enc) + bytes(nbytes)
    return struct.pack("<II", 10, len(body) if says is None else says) + body


HEAD = b"LFVT" + struct.pack("<I", 1)
FEATURES = struct.pack("<II", 2, 12) + struct.pack("<dI", 1.0, 0)
MALFORMED = {
    "shorter than its header": struct.pack("<II", 10, 10) + bytes(10),
    "fewer pixels than height x step": image_record(nbytes=16 * 32 - 1),
    "more pixels than height x step": image_record(nbytes=16 * 32 + 1),
    "the file ends inside the pixels": image_record(nbytes=100, says=24 + 16 * 32),
    "step < width": image_record(w=32, step=31),
    "width 15": image_record(w=15),
    "width 8193": image_record(w=8193, h=16),
    "height 15": image_record(h=15),
    "height 8193": image_record(w=16, h=8193),
    "an unknown encoding": image_record(enc=1),
    "images of differing size": image_record() + image_record(t=1.1, w=48),
    "images of differing height": image_record() + image_record(t=1.1, h=17),
    "feature messages and raw images": FEATURES + image_record(),
    "raw images and feature messages": image_record() + FEATURES,
}


def test_malformed_image_records_are_refused(host, oracle, tmp_path):
    from lfvio.host import HostEstimator

    cpu = HostEstimator(oracle.build_host_oracle())
    assert not cpu.has_tracker  # the suite's CPU build has no image route, and still loads
    try:
        good = str(tmp_path / "good.lfvt")
        open(good, "wb").write(HEAD + image_record() + image_record(t=1.1, step=40))
        assert host.replay(good)[0] == 0 and cpu.replay(good)[0] == 0 and host.trace_raw_images(good)[0] == 2
        for name, body in MALFORMED.items():
            p = str(tmp_path / "bad.lfvt")
            open(p, "wb").write(HEAD + body)
            assert host.replay(p)[0] == -3, name
            assert cpu.replay(p)[0] == -3, name
            n, _, err = host.trace_raw_images(p)
            assert n == -3 and err, name
        with pytest.raises(RuntimeError):
            cpu.track_trace(good, str(tmp_path / "out.lfvt"))
    finally:
        cpu.close()


def test_existing_replay_sees_no_images_in_a_raw_recording(host, tmp_path):
    """Today's behaviour, restated: to replay() a raw image is a record of a type it does not know."""
    p = str(tmp_path / "raw.lfvt")
    made = trace.make_image_stream(p, seed=3, n_frames=13, scale=16)
    assert len(made["stamps"]) == 13
    host.clear_state()
    rc, st = host.replay(p, "")
    assert rc == 0 and st["images"] == 0 and st["poses"] == 0 and st["bootstraps"] == 0 and st["last_status"] == 0


def test_make_image_stream_tiny(tmp_path):
    from lfvio.engine import annulus_mask

    p = str(tmp_path / "tiny.lfvt")
    n = 14
    made = trace.make_image_stream(p, seed=1, n_frames=n, scale=16)
    t = trace.read_trace(p)
    W, H = made["width"], made["height"]
    assert (W, H) == (80, 60) and len(t["raw_images"]) == n and not t["images"] and len(t["bootstraps"]) == 1
    # the clock: exposure at 0.1 k + cam_offset, stamped that minus TD0
    stamps = [s for s, _ in t["raw_images"]]
    assert np.allclose(stamps, [0.1 * k + 0.0023 - synth.TD0 for k in range(n)], rtol=0, atol=1e-12) and stamps == made["stamps"]
    assert np.array_equal(t["truth"][:, 0], stamps)
    # the order: IMU samples up to the first one behind an image, the image, its truth; the bootstrap record in front of image 12
    order = t["order"]
    pos = [i for i, k in enumerate(order) if k == trace.REC_IMAGE]
    assert all(order[i + 1] == trace.REC_TRUTH for i in pos)
    assert order.index(trace.REC_BOOTSTRAP) == pos[12] - 1 and order.count(trace.REC_BOOTSTRAP) == 1
    imu_before = [sum(1 for k in order[:i] if k == trace.REC_IMU) for i in pos]
    for k, c in enumerate(imu_before):
        exposure = 0.1 * k + 0.0023
        assert t["imu"][c - 1, 0] > exposure and t["imu"][c - 2, 0] <= exposure, k  # exactly one sample behind the image
    # the stamped bootstrap: the window of the first eleven published messages, raw images 2 .. 12
    b = t["bootstraps"][0]
    assert b.size == 248 and b[247] == stamps[12] and made["first_window"] == 2
    truth = made["truth"]
    assert np.abs(b[:33].reshape(11, 3) - np.array([truth[k][1] for k in range(2, 13)])).max() < 0.1  # (2 cm noise)
    # the pictures: black outside the 40 - 120 degree window, lit inside, and the base mask inside the window
    cam = made["camera"]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = u - cam["cx"], v - cam["cy"]
    phi = np.hypot(x, y)
    z = sum(c * phi ** i for i, c in enumerate(cam["poly"]))
    ang = np.degrees(np.arctan2(phi, -z))
    inside = (ang >= 40.0) & (ang <= 120.0)
    mask = annulus_mask(W, H, *made["annulus"]) > 0
    assert 0.3 < inside.mean() < 0.8 and mask.sum() > 0.4 * inside.sum() and not (mask & ~inside).any()
    for _, img in t["raw_images"]:
        assert not img[~inside].any() and img[inside].min() >= 1 and img[inside].std() > 15.0
    assert not np.array_equal(t["raw_images"][0][1], t["raw_images"][5][1])
    # seeded
    q = str(tmp_path / "again.lfvt")
    trace.make_image_stream(q, seed=1, n_frames=n, scale=16)
    assert open(p, "rb").read() == open(q, "rb").read()
    assert abi.NUM_FRAMES == 11


def test_bag_with_an_image_topic(tmp_path):
    import bag_to_lfvt

    bag, out = str(tmp_path / "cam.bag"), str(tmp_path / "cam.lfvt")
    imgs = [picture(10 + k, 48, 32) for k in range(5)]
    w = rosmsg.BagWriter(bag, chunk_messages=4)
    for k, img in enumerate(imgs):
        t = 100.0 + 0.1 * k
        w.write("/imu0", "sensor_msgs/Imu", t - 0.02, rosmsg.ser_imu(k, t - 0.02, [0.1 * k, 0.0, 9.8], [0.0, 0.01, 0.0]))
        w.write("/cam0/image_raw", "sensor_msgs/Image", t + 0.003, rosmsg.ser_image(k, t, img, step=None if k % 2 else 64, encoding=b"8UC1" if k == 3 else b"mono8"))
        w.write("/feature_tracker/feature", "sensor_msgs/PointCloud", t + 0.02, rosmsg.ser_pointcloud(k, t, np.zeros((2, 9), np.float32)))
    w.write("/feature_tracker/restart", "std_msgs/Bool", 100.6, rosmsg.ser_bool(True))
    w.close()
    st, img, step, enc = rosmsg.de_image(rosmsg.ser_image(7, 12.25, imgs[0], step=50))
    assert (st, step, enc) == (12.25, 50, "mono8") and np.array_equal(img, imgs[0])
    with pytest.raises(ValueError):
        rosmsg.de_image(rosmsg.ser_image(7, 12.25, imgs[0], encoding=b"bgr8"))
    n = bag_to_lfvt.convert(bag, out, image_topic="/cam0/image_raw")
    assert n["raw_images"] == 5 and n["imu"] == 5 and n["images"] == 0 and n["restarts"] == 0 and n["other"] == 6
    t = trace.read_trace(out)
    assert t["order"] == [1, 10] * 5 and t["raw_steps"] == [64, 48, 64, 48, 64]
    for k, (stamp, img) in enumerate(t["raw_images"]):
        assert abs(stamp - (100.0 + 0.1 * k)) < 1e-9 and np.array_equal(img, imgs[k])
    # without the option the bag converts as before: the feature topic, no raw images
    n = bag_to_lfvt.convert(bag, out)
    assert n["images"] == 5 and n["restarts"] == 1 and "raw_images" not in n and n["other"] == 5


def table(n, seed=0):
    rng = np.random.default_rng(seed)
    return dict(pts=rng.uniform(0, 300, (n, 2)).astype(np.float32), ids=rng.permutation(n).astype(np.int32) + 7,
                cnt=rng.integers(1, 6, n).astype(np.int32), un3d=rng.normal(size=(n, 3)).astype(np.float32),
                vel=rng.normal(size=(n, 3)).astype(np.float32))


def by_hand(t):
    rows = []
    for i in range(len(t["ids"])):
        if t["cnt"][i] > 1:
            rows.append([t["un3d"][i, 0], t["un3d"][i, 1], t["un3d"][i, 2], np.float32(int(t["ids"][i]) * 1 + 0), t["pts"][i, 0], t["pts"][i, 1],
                         t["vel"][i, 0], t["vel"][i, 1], t["vel"][i, 2]])
    return np.array(rows, np.float32).reshape(-1, 9)


@pytest.mark.parametrize("n", [0, 17, 4096])
def test_rows_from_table(n):
    t = table(n, seed=n)
    r = nr.rows_from_table(**t)
    assert r.dtype == np.float32 and r.shape == (int((t["cnt"] > 1).sum()), 9) and r.tobytes() == by_hand(t).tobytes()
    if n:
        assert 0 < len(r) < n
        assert np.array_equal(r[:, 3], t["ids"][t["cnt"] > 1].astype(np.float32))  # table order kept
    ones = dict(t, cnt=np.ones(n, np.int32))
    assert nr.rows_from_table(**ones).shape == (0, 9)
    full = dict(t, cnt=np.full(n, 2, np.int32))
    assert nr.rows_from_table(**full).tobytes() == by_hand(full).tobytes() and len(nr.rows_from_table(**full)) == n


def test_rows_round_an_id_to_the_nearest_even_float():
    t = table(4)
    t["ids"] = np.array([16777217, 16777219, 2 ** 31 - 1, 5], np.int32)  # 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4
    t["cnt"][:] = 3
    r = nr.rows_from_table(**t)
    assert r[:, 3].tolist() == [16777216.0, 16777220.0, 2147483648.0, 5.0]
