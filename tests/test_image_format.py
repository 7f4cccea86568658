"""Colour and 16-bit camera images on the device (lfvio_image_format_set, lfvio_image_gray, lfvio_track_batch_format): every call
under a format equals, bit for bit, the same call without one on the converted image (tests/image_ref.py: the specification).  No
tolerance anywhere.

The images are the 80 x 60 frames of trace.make_image_stream(scale=16) and a few odd shapes.  Raw images are made from grey ones by
image_ref.from_gray, so that texture survives; their grey twin is image_ref.to_gray of the result.

  1  lfvio_image_gray against image_ref for every code at five shapes, the padding noisy, the input once at an odd address (the
     staging block realigns the image's first byte on the device, so it is the steps that are no multiple of 4 and the widths
     17 that take the kernel's byte path there; (16, 16, 0), the 512-byte step and 80 x 60 at whole steps take the wide path)
  2  lfvio_klt_track: format on one context, the grey twins on another; CLAHE on; the setting survives the reset, NULL takes it off, a
     mono8 format with step = width equals none
  3  lfvio_track_frame_message: four publishing frames, bgr8 with step 3 w + 5 and mono16 with step 2 w, CLAHE off and on
  4  lfvio_track_batch_frame: three slots, one idle in the second call, rgba8 with padded rows; the atomic refusal of a short step
  5  refusals on every route leave pre-filled outputs alone
  6  the host route: a recording as bgr8 records and as the mono8 records of its grey twin give the same trajectory file"""
import ctypes as C
import struct

import numpy as np
import pytest

import image_ref as ir
from test_track_batch import sentinels, untouched
from test_tracker_chain import same

pytestmark = pytest.mark.gpu

W, H, S = 80, 60, 50
KW = dict(max_count=40, min_distance=6, mask_radius=6, win_size=15, width=W, height=H)
TABLE = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")
SCALARS = ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject", "num_rows")
SHAPES = [(16, 16, 0), (17, 19, 1), (17, 19, 3), (64, 48, 5), (80, 60, None)]  # (w, h, step - w * bpp; None: step 512)


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """Six 80 x 60 frames of the rendered stream and its camera: made once, shared, never changed."""
    from lfvio import trace

    p = str(tmp_path_factory.mktemp("imgfmt") / "s.lfvt")
    made = trace.make_image_stream(p, seed=2, n_frames=6, scale=16)
    assert (made["width"], made["height"]) == (W, H)
    return [img for _, img in trace.read_trace(p)["raw_images"]], made["camera"]


@pytest.fixture(scope="module")
def twin():
    from lfvio.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def words(k):
    return np.random.default_rng([k, 9]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def raws(frames, code, step, seed=0):
    """-> (the raw rows, their grey twins)"""
    rows = [ir.from_gray(g, code, step, seed=seed + k) for k, g in enumerate(frames)]
    return rows, [ir.to_gray(r, W, code) for r in rows]


def everything(r):
    rj, dt = r["reject"], r["detect"]
    parts = [np.ascontiguousarray(r[key]).tobytes() for key in TABLE + ("rows",)]
    parts.append(repr([r[key] for key in SCALARS] + [r["rc"], rj["status"], rj["best_sample"], rj["num_inliers"], dt["num_kept"], dt["num_corners"],
                                                     dt["num_candidates"]]).encode())
    parts += [np.float64(rj["best_score"]).tobytes(), np.ascontiguousarray(rj["E"]).tobytes(), np.float64(dt["max_response"]).tobytes()]
    for key, v in sorted(r.get("stages", {}).items()):
        parts.append(key.encode() + (b"-" if v is None else np.ascontiguousarray(v).tobytes()))
    return parts


def levels(e):
    out = []
    for k in range(6):
        px = e.klt_level(k, check=False)
        if px is None:
            break
        out.append(px)
    return out


def setup(e, code=None, step=0, clahe=False):
    e.track_frame_reset()
    e.gft_set_mask(None)
    e.clahe_set(3.0, (8, 8)) if clahe else e.clahe_set(None)
    e.image_format(code, step)


# ---- 1
@pytest.mark.parametrize("code", ir.CODES)
def test_image_gray(eng, code):
    bpp = ir.BPP[code]
    for w, h, pad in SHAPES:
        step = 512 if pad is None else w * bpp + pad
        rows = np.random.default_rng(1000 * code + 10 * w + step).integers(0, 256, (h, step), dtype=np.uint8)
        want = ir.to_gray(rows, w, code)
        got = eng.image_gray(rows, w, h, code, step)
        assert same(got, want), (code, w, h, step)
        # the same bytes from an odd address inside a larger array
        big = np.zeros(h * step + 8, np.uint8)
        big[1:1 + h * step] = rows.ravel()
        assert big[1:].ctypes.data - big.ctypes.data == 1
        assert same(eng.image_gray(big[1:1 + h * step], w, h, code, step), want), (code, w, h, step, "offset")
        if pad == 0:  # step 0 means the pixels alone
            assert same(eng.image_gray(rows, w, h, code, 0), want)
    flat = np.random.default_rng(code).integers(0, 256, (H, W), dtype=np.uint8)
    assert same(eng.image_gray(flat, W, H), flat)  # a null format: mono8, rows contiguous


# ---- 2
def flow(e, imgs, pts, **kw):
    """Two consecutive images: the first makes itself resident, the second tracks `pts`.  -> everything that came back, and the pyramid."""
    e.klt_reset()
    a = e.klt_track(imgs[0], np.zeros((0, 2), np.float32), win_size=11, size=(W, H), **kw)
    b = e.klt_track(imgs[1], pts, win_size=11, size=(W, H), **kw)
    return [b["next"].tobytes(), b["status"].tobytes(), b["iterations"].tobytes(), repr((a["levels_used"], b["levels_used"], b["num_tracked"], a["rc"], b["rc"]))], levels(e), b


@pytest.fixture(scope="module")
def points(stream, twin):
    frames, _ = stream
    setup(twin)
    twin.klt_track(frames[0], np.zeros((0, 2), np.float32))
    pts = twin.gft_detect(None, None, max_count=30, min_distance=5, mask_radius=5)["corners"].copy()
    assert 20 <= len(pts) <= 30
    return pts


@pytest.mark.parametrize("clahe", [False, True])
@pytest.mark.parametrize("code,pad", [(ir.BGR8, 5), (ir.MONO16, 0), (ir.RGBA8, 8), (ir.MONO16_BE, 3), (ir.RGB8, 0), (ir.BGRA8, 1), (ir.MONO8, 7)])
def test_klt_track(eng, twin, stream, points, code, pad, clahe):
    frames, _ = stream
    step = W * ir.BPP[code] + pad
    rows, grey = raws(frames[:2], code, step, seed=code)
    setup(eng, code, step, clahe)
    setup(twin, None, 0, clahe)
    got, got_levels, b = flow(eng, rows, points)
    want, want_levels, _ = flow(twin, grey, points)
    assert got == want
    assert len(got_levels) == len(want_levels) == 3 and all(same(x, y) for x, y in zip(got_levels, want_levels))
    assert b["levels_used"] == 2 and b["num_tracked"] >= 10
    if not clahe:
        assert same(got_levels[0], grey[1])  # level 0 is the grey image
    else:
        assert not same(got_levels[0], grey[1]) and same(got_levels[0], twin.clahe_apply(grey[1], 3.0, (8, 8)))
    # the setting survives the reset; NULL takes it off
    eng.klt_reset()
    again, _, _ = flow(eng, rows, points)
    assert again == want
    eng.image_format(None)
    off, off_levels, _ = flow(eng, grey, points)
    assert off == want and same(off_levels[0], want_levels[0])


def test_mono8_format_with_step_width_equals_none(eng, twin, stream, points):
    frames, _ = stream
    setup(twin)
    want, want_levels, _ = flow(twin, frames[:2], points)
    for step in (W, 0):
        setup(eng, ir.MONO8, step)
        got, got_levels, _ = flow(eng, frames[:2], points)
        assert got == want and all(same(x, y) for x, y in zip(got_levels, want_levels))


# ---- 3
def message_run(e, imgs, cam):
    out = []
    for k, img in enumerate(imgs):
        r = e.track_frame_message(img, 5.0 + 0.1 * k, cam, publish=True, words=words(k), stages=True, **KW)
        out.append((everything(r), [x.tobytes() for x in levels(e)], r))
    return out


@pytest.mark.parametrize("clahe", [False, True])
@pytest.mark.parametrize("code,pad", [(ir.BGR8, 5), (ir.MONO16, 0)])
def test_track_frame_message(eng, twin, stream, code, pad, clahe):
    frames, cam = stream
    step = W * ir.BPP[code] + pad
    rows, grey = raws(frames[:4], code, step, seed=10 + code)
    setup(eng, code, step, clahe)
    setup(twin, None, 0, clahe)
    got, want = message_run(eng, rows, cam), message_run(twin, grey, cam)
    for k in range(4):
        assert got[k][0] == want[k][0], k
        assert got[k][1] == want[k][1] and len(got[k][1]) >= 1, k
    last = got[3][2]
    assert last["num_points"] >= 15 and last["num_rows"] >= 8 and last["num_tracked"] >= 8 and last["velocity_3d"].any()
    # the setting survives lfvio_track_frame_reset
    eng.track_frame_reset()
    assert message_run(eng, rows[:2], cam)[1][0] == want[1][0]


# ---- 4
def alone(entries, cam, clahe):
    from lfvio.engine import Engine

    e = Engine(0)
    try:
        setup(e, None, 0, clahe)
        return [None if f is None else e.track_frame_message(f["img"], f["time"], cam, publish=True, words=f["words"], **KW) for f in entries]
    finally:
        e.close()


def test_track_batch_frame(eng, stream):
    frames, cam = stream
    code, step = ir.RGBA8, 4 * W + 8
    cols_raw, cols_grey = [], []
    for slot in range(3):
        rows, grey = raws(frames[slot:slot + 3], code, step, seed=40 + 10 * slot)
        cols_raw.append([dict(img=r, time=7.0 + 0.1 * k, cam=cam, words=words(10 * slot + k)) for k, r in enumerate(rows)])
        cols_grey.append([dict(img=g, time=7.0 + 0.1 * k, words=words(10 * slot + k)) for k, g in enumerate(grey)])
    cols_raw[1][1] = cols_grey[1][1] = None  # slot 1 idle in the second call
    try:
        for clahe in (False, True):
            eng.track_batch_reserve(3)
            eng.track_batch_clahe(3.0, (8, 8)) if clahe else eng.track_batch_clahe(None)
            eng.track_batch_format(code, step)
            got = [eng.track_batch_frame([col[k] for col in cols_raw], **KW) for k in range(2)]
            # the atomic refusal: a step below 4 w, outputs pre-filled
            eng.track_batch_format(code, 4 * W - 1)
            bufs = sentinels(3)
            res = eng.track_batch_frame([col[2] for col in cols_raw], buffers=bufs, check=False, **KW)
            assert res[0]["rc"] == -1 and untouched(bufs, res)
            eng.track_batch_format(code, step)
            got.append(eng.track_batch_frame([col[2] for col in cols_raw], **KW))
            for slot in range(3):
                want = alone(cols_grey[slot], cam, clahe)
                for k in range(3):
                    if want[k] is None:
                        assert got[k][slot]["num_points"] == 0 and got[k][slot]["num_rows"] == 0
                    else:
                        assert everything(got[k][slot]) == everything(want[k]), (clahe, slot, k)
                assert got[2][slot]["num_points"] >= 15 and got[2][slot]["num_tracked"] >= 8
        # the setting is the batch's: NULL takes it off, and the grey twins then give the same bits
        eng.track_batch_reserve(3)
        eng.track_batch_format(None)
        plain = eng.track_batch_frame([dict(col[0], cam=cam) for col in cols_grey], **KW)
        assert all(everything(plain[slot]) == everything(got[0][slot]) for slot in range(3))
    finally:
        eng.track_batch_format(None)
        eng.track_batch_clahe(None)
        eng.track_batch_reserve(0)


# ---- 5
def test_refusals_on_every_route(eng, stream):
    from lfvio import abi

    frames, cam = stream
    up = C.POINTER(C.c_ubyte)
    # the settings: a code outside the table, a step outside its range; the previous setting stays
    setup(eng, ir.BGR8, 3 * W + 5)
    for code, step in ((1, 0), (8, 0), (-1, 0), (ir.BGR8, 65537), (ir.BGR8, -1)):
        assert eng.image_format(code, step, check=False) == -1 and eng.track_batch_format(code, step, check=False) == -1, (code, step)
    assert eng.lib.lfvio_image_format_set(None, None) == -1 and eng.lib.lfvio_track_batch_format(None, None) == -1
    rows, grey = raws(frames[:2], ir.BGR8, 3 * W + 5, seed=3)
    want = eng.klt_track(rows[0], np.zeros((0, 2), np.float32), size=(W, H))  # (the bgr8 setting is still on)
    assert want["rc"] == 0 and same(eng.klt_level(0), grey[0])
    # lfvio_image_gray
    big = np.zeros((H, 65537), np.uint8)
    for code, step in ((1, 0), (8, 0), (ir.BGR8, 65537), (ir.BGR8, 3 * W - 1), (ir.MONO8, W - 1), (ir.MONO16, 2 * W - 1), (ir.RGBA8, 4 * W - 1)):
        out = np.full((H, W), 0xA5, np.uint8)
        rc, _ = eng.image_gray(big, W, H, code, step, out=out, check=False)
        assert rc == -1 and (out == 0xA5).all(), (code, step)
    out = np.full((H, W), 0xA5, np.uint8)
    assert eng.image_gray(None, W, H, ir.BGR8, 0, out=out, check=False)[0] == -1 and eng.image_gray(big, 15, H, ir.BGR8, 0, out=out, check=False)[0] == -1
    assert eng.lib.lfvio_image_gray(eng.ctx, None, W, H, big.ctypes.data_as(up), None) == -1 and (out == 0xA5).all()
    # the calls that take an image, at a step below the row: outputs and the resident image untouched
    for code in (ir.BGR8, ir.MONO8, ir.MONO16, ir.RGBA8):
        eng.image_format(code, W * ir.BPP[code] - 1)
        nxt, stat = np.full((4, 2), 7.5, np.float32), np.full(4, 77, np.uint8)
        r = eng.klt_track(big, np.full((4, 2), 20.0, np.float32), next=nxt, status=stat, size=(W, H), check=False)
        assert r["rc"] == -1 and (nxt == 7.5).all() and (stat == 77).all() and same(eng.klt_level(0), grey[0]), code
        bufs = sentinels(1)
        arrays, o, rows_out = bufs[0]
        m = abi.TrackMessageC()
        m.num_rows = -77
        r = eng.track_frame_message(big, 9.0, cam, publish=True, words=words(0), out=o, arrays=arrays, rows=rows_out, msg=m, check=False, **KW)
        assert r["rc"] == -1 and untouched(bufs, [dict(msg_num_rows=int(m.num_rows))]) and same(eng.klt_level(0), grey[0]), code
    # and the next good call gives the bits it would have given
    eng.image_format(ir.BGR8, 3 * W + 5)
    a = eng.klt_track(rows[1], np.full((4, 2), 30.0, np.float32), size=(W, H))
    setup(eng)
    eng.klt_track(grey[0], np.zeros((0, 2), np.float32))
    b = eng.klt_track(grey[1], np.full((4, 2), 30.0, np.float32))
    assert a["next"].tobytes() == b["next"].tobytes() and a["status"].tobytes() == b["status"].tobytes()


# ---- 6
def reencode(src, dst, code):
    """The recording `src` (mono8 records) with every image as a `code` record (code 0: the mono8 record of that raw image's grey twin)."""
    body = open(src, "rb").read()
    out, o, k = [body[:8]], 8, 0
    while o < len(body):
        kind, n = struct.unpack_from("<II", body, o)
        p = body[o + 8:o + 8 + n]
        o += 8 + n
        if kind == 10:
            t, w, h, step, enc = struct.unpack("<dIIII", p[:24])
            assert enc == 0
            grey = np.frombuffer(p[24:], np.uint8).reshape(h, step)[:, :w]
            raw = ir.from_gray(grey, ir.BGR8, 3 * w + 4, seed=k)
            rows = raw if code else ir.to_gray(raw, w, ir.BGR8)
            p = struct.pack("<dIIII", t, w, h, rows.shape[1], code) + rows.tobytes()
            k += 1
        out.append(struct.pack("<II", kind, len(p)) + p)
    open(dst, "wb").write(b"".join(out))
    return k


def test_host_route(tmp_path):
    """36 frames at scale 4, the settings of tests/test_image_replay.py's pixels-to-poses replay."""
    from lfvio import trace
    from lfvio.host import HostEstimator

    src = str(tmp_path / "grey.lfvt")
    made = trace.make_image_stream(src, seed=0, n_frames=36, scale=4)
    paths = {code: str(tmp_path / f"enc{code}.lfvt") for code in (ir.BGR8, ir.MONO8)}
    for code, p in paths.items():
        assert reencode(src, p, code) == 36
    out = {}
    for code, p in paths.items():
        he = HostEstimator()
        try:
            assert he.trace_raw_encoding(p) == code
            he.clear_state()
            he.set_min_parallax(10.0)
            he.set_solver_time(0.0)
            he.track_config(made["camera"], max_cnt=80, min_dist=12, freq=10, num_samples=100, seed=77, annulus=made["annulus"])
            traj = str(tmp_path / f"traj{code}.txt")
            rc, st, ts = he.replay_images(p, traj)
            out[code] = (rc, st, {k: v for k, v in ts.items() if k != "tracker_ms"}, open(traj, "rb").read())
        finally:
            he.close()
    assert out[ir.BGR8] == out[ir.MONO8]
    rc, st, ts, traj = out[ir.BGR8]
    assert rc == 0 and st["bootstraps"] == 1 and st["last_status"] == 0 and st["poses"] > 0 and len(traj) > 0, st
    assert ts["raw_images"] == 36 and ts["published"] == 34 and ts["rows"] > 0  # (the gate publishes by the stamps alone)
