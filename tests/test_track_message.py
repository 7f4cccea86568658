"""lfvio_track_frame_message on the device: everything lfvio_track_frame gives, bit for bit, on a second context fed the same words,
and the rows of the node's feature message equal to node_ref.rows_from_table of the call's own outputs.  The images are the
161 x 123 six-frame sequence of tests/test_tracker_chain.py with the settings of tests/test_track_frame.py.

  1  six frames through track_frame on one engine and track_frame_message on another: out, stages and (through the frames that
     follow) all resident state equal; the rows; frame 0 gives none (every count is 1)
  2  publish off: no rows, a 0x5A-filled rows buffer untouched
  3  grey frames that empty the table: no rows
  4  max_count 4096 on a 320 x 240 noise texture, more than 2048 rows in the second frame and a count that is no multiple of 16
  5  refused calls (msg null, rows null, one of track_frame's own): everything untouched, the next frame as if they never happened
  6  a frame beside an optimization in flight"""
import ctypes as C

import numpy as np
import pytest

from node_ref import rows_from_table
from test_tracker_chain import CAM, same
from test_track_frame import KW, S, TABLE, flat, plain, sentinel, when, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def imgs():
    from test_tracker_chain import frames

    return frames()


@pytest.fixture(scope="module")
def other():
    from lfvio.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def call(e, img, k, message, publish=True, kw=KW, **more):
    f = e.track_frame_message if message else e.track_frame
    return f(img, when(k), CAM, publish=publish, words=words(k), stages=True, **dict(kw, **more))


def equal_frames(a, b, tag):
    """Everything track_frame returns, from two calls."""
    for key in TABLE:
        assert same(a[key], b[key]), (tag, key)
    for key in ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject", "rc"):
        assert a[key] == b[key], (tag, key)
    assert repr(a["detect"]) == repr(b["detect"]), tag
    for key in ("status", "best_sample", "num_inliers"):
        assert a["reject"][key] == b["reject"][key], (tag, key)
    assert np.float64(a["reject"]["best_score"]).tobytes() == np.float64(b["reject"]["best_score"]).tobytes() and same(a["reject"]["E"], b["reject"]["E"]), tag
    for key, v in a["stages"].items():
        w = b["stages"][key]
        assert (v is None and w is None) or same(v, w), (tag, "stages", key)


def own_rows(r):
    return rows_from_table(r["pts"], r["ids"], r["track_cnt"], r["un_pts_3d"], r["velocity_3d"])


def test_six_frames_equal_track_frame_and_the_rows(eng, other, imgs):
    """Test 1."""
    for e in (eng, other):
        plain(e)
        e.track_frame_reset()
    total = 0
    for k, img in enumerate(imgs):
        a, b = call(eng, img, k, False), call(other, img, k, True)
        equal_frames(a, b, k)
        assert same(b["rows"], own_rows(b)) and b["num_rows"] == int((b["track_cnt"] > 1).sum()), k
        total += b["num_rows"]
        if k == 0:
            assert b["num_rows"] == 0 and b["num_points"] >= 20 and np.all(b["track_cnt"] == 1)
        else:
            assert 10 <= b["num_rows"] <= b["num_points"], k
    assert any(0 < int((r > 1).sum()) < len(r) for r in [b["track_cnt"]])  # rows and non-rows in one table
    # the resident state once more, with the routes exchanged
    a, b = call(eng, imgs[0], 6, True), call(other, imgs[0], 6, False)
    equal_frames(b, a, "exchanged")
    assert same(a["rows"], own_rows(a)) and total > 0


def test_publish_off_writes_no_rows(eng, imgs):
    """Test 2."""
    plain(eng)
    eng.track_frame_reset()
    call(eng, imgs[0], 0, True)
    r1 = call(eng, imgs[1], 1, True)
    assert r1["num_rows"] > 10
    buf = np.full((4096, 9), np.frombuffer(b"\x5a" * 4, np.float32)[0], np.float32)
    r2 = eng.track_frame_message(imgs[2], when(2), CAM, publish=False, words=None, num_samples=S, rows=buf, **KW)
    assert r2["rc"] == 0 and r2["num_rows"] == 0 and buf.tobytes() == b"\x5a" * buf.nbytes
    assert r2["num_points"] == r2["num_tracked"] > 8 and int((r2["track_cnt"] > 1).sum()) > 8  # (a publishing call would have had rows)


def test_grey_frames_that_empty_the_table(eng, imgs):
    """Test 3."""
    plain(eng)
    eng.track_frame_reset()
    grey = np.full_like(imgs[0], 117)
    ress = [call(eng, img, k, True) for k, img in enumerate([imgs[0], imgs[1], grey, grey, imgs[3]])]
    for k, r in enumerate(ress):
        assert same(r["rows"], own_rows(r)), k
    assert ress[1]["num_rows"] > 10 and ress[3]["num_points"] == 0 and ress[3]["num_rows"] == 0
    assert ress[4]["num_rows"] == 0 and ress[4]["num_points"] >= 20  # filled again: every count is 1
    # a grey first frame: an empty table at the start and at the end of the call
    eng.track_frame_reset()
    r = call(eng, grey, 0, True)
    assert (r["num_points"], r["num_rows"]) == (0, 0)


BIG_W, BIG_H, BIG_SEED = 320, 240, 1


def noise_frames():
    """Two 320 x 240 windows, one pixel apart, of a seeded noise image smoothed by [1 2 1] / 4 both ways: thousands of corners."""
    rng = np.random.default_rng([BIG_SEED, 77])
    a = rng.integers(0, 256, (BIG_H + 8, BIG_W + 8)).astype(np.float64)
    k = np.array([1.0, 2.0, 1.0]) / 4.0
    a = sum(k[i] * np.roll(a, i - 1, 0) for i in range(3))
    a = sum(k[i] * np.roll(a, i - 1, 1) for i in range(3))
    a = np.clip(np.rint((a - a.mean()) * 2.2 + 127.5), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(a[4:4 + BIG_H, 4 + d:4 + d + BIG_W]) for d in (0, 1)]


def test_a_full_table(eng, other):
    """Test 4: rows from more than half of the threads of the scan, the last one with a part of its sixteen."""
    from lfvio import synth

    cam = dict(CAM, cx=160.5, cy=123.0, poly=tuple(c * 4.0 ** i / 4.0 for i, c in enumerate(synth.OCAM_POLY)))  # the PAL camera, 4 times smaller
    kw = dict(KW, max_count=4096, min_distance=3, mask_radius=3)
    f0, f1 = noise_frames()
    for e in (eng, other):
        plain(e)
        e.track_frame_reset()
    res = []
    for k, img in enumerate((f0, f1)):
        a = eng.track_frame(img, when(k), cam, words=words(k), stages=True, **kw)
        b = other.track_frame_message(img, when(k), cam, words=words(k), stages=True, **kw)
        equal_frames(a, b, ("big", k))
        assert same(b["rows"], own_rows(b)), k
        res.append(b)
    print("full table:", [(r["num_points"], r["num_rows"]) for r in res])
    assert res[0]["num_points"] > 2048 and res[0]["num_rows"] == 0
    n = res[1]["num_rows"]
    assert n > 2048 and n % 16 != 0 and res[1]["num_points"] > n


def test_refused_calls_leave_everything(eng, imgs):
    """Test 5."""
    from lfvio import abi

    plain(eng)
    eng.track_frame_reset()
    want = [call(eng, img, k, True) for k, img in enumerate(imgs[:3])]
    eng.track_frame_reset()
    for k, img in enumerate(imgs[:2]):
        call(eng, img, k, True)
    fill = np.frombuffer(b"\x5a" * 4, np.float32)[0]
    for bad in (dict(msg=None), dict(rows=False), dict(width=15), dict(capacity=3)):
        arrays, out = sentinel()
        head = bytes(out)[:abi.TrackFrameOutC.pts.offset]
        m = abi.TrackMessageC()
        C.memset(C.byref(m), 0x5A, C.sizeof(m))
        buf = np.full((4096, 9), fill, np.float32)
        a = dict(msg=m, rows=buf)
        a.update(bad)
        r = eng.track_frame_message(imgs[2], when(2), CAM, words=words(2), arrays=arrays, out=out, check=False, **dict(KW, **a))
        assert r["rc"] == -1, bad
        assert bytes(out)[:len(head)] == head and all(np.all(v == (77 if v.dtype == np.int32 else 7.5)) for v in arrays.values()), bad
        assert buf.tobytes() == b"\x5a" * buf.nbytes, bad
        if a["msg"] is not None and a["rows"] is not False:
            assert bytes(m)[:4] == b"\x5a" * 4, bad  # num_rows
    fin, out, m = abi.TrackFrameInC(), abi.TrackFrameOutC(), abi.TrackMessageC()
    assert eng.lib.lfvio_track_frame_message(None, C.byref(fin), C.byref(out), None, C.byref(m)) == -1
    # nothing resident moved
    got = call(eng, imgs[2], 2, True)
    equal_frames(got, want[2], "after the refused calls")
    assert same(got["rows"], want[2]["rows"]) and got["num_rows"] > 10 and got["velocity_3d"].any()


def test_beside_an_optimization_in_flight(eng, imgs):
    """Test 6."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    def three(e):
        plain(e)
        e.track_frame_reset()
        return [call(e, img, k, True) for k, img in enumerate(imgs[:3])]

    alone = three(eng)
    w = synth.make_window(0, 300)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    e0, e1 = Engine(0), Engine(0)
    try:
        sol0, prior0, _ = split(e0, None)
        sol1, prior1, ress = split(e1, three)
    finally:
        e0.close()
        e1.close()
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and np.array_equal(sol0.lam, sol1.lam)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert flat(ress) == flat(alone)
    for a, b in zip(alone, ress):
        assert same(a["rows"], b["rows"])
    assert ress[2]["num_rows"] > 10
