"""Tracking on the EXPANDED image on the device (lfvio_track_source_set, k_remap_gray, LFVIO_CAM_EQUIRECT).  The contract,
bit for bit and without a tolerance anywhere: a context with the setting on gives, for every output of lfvio_klt_track, lfvio_track_frame
and lfvio_track_frame_message and for lfvio_klt_level afterwards, what a second context gives that is fed lfvio_remap_apply's output
under lfvio_image_format_set({the same encoding, step 0}).

Sources are 161 x 123 noise with a padded odd step, or the 320 x 240 frames of trace.make_image_stream(scale=4); outputs are 131 x 67
(8777 pixels, 1 mod 4: the last lane's tail) and 128 x 64.

  1  level 0 after one lfvio_klt_track equals the numpy chain (image_ref.to_gray of project_ref.remap) for mono8, bgr8, rgb8, bgra8 and
     mono16 of both byte orders, both output sizes, an equirectangular map through an OCam camera and a perspective map through a pinhole
     camera whose M sends part of the output outside the source; the map is first shown, on the CPU, to have inside AND outside entries
  2  chain equality: six frames of the rendered stream through each of the three calls, CLAHE off and on — every array, the counts, the
     message rows and all pyramid levels
  3  the integer map's owner: the source's step changes between frames and lfvio_remap_apply of another encoding and geometry, and an
     lfvio_cloud_fuse with LFVIO_FUSE_IMAGE_REMAP, run in between; everybody still equals their own reference
  4  refusals (LFVIO_ERR_ARG with a message, pre-filled outputs and the resident image untouched): no map, a map of another size, a
     source side of 15 or 8193, a step too small for src_width, the setting on after lfvio_remap_reset; the next good call gives the
     bytes of a context that never saw the refused ones
  5  off again: after lfvio_track_source_set(NULL) plain frames give the bytes of a fresh context
  6  the lift: lfvio_track_undistort and lfvio_track_reject with model 6 at N = 37 and N = 200 equal equirect_ref bit for bit — the
     bearings, status[], the winner and the count, every output of undistortedPoints; E and the score against the device's own two-view
     path on equirect_ref's bearings, as tests/test_track.py holds every other model (numpy's E is LAPACK's SVD: nobody's bits); one
     lfvio_track_batch_frame slot with a model-6 camera equals a context of its own; the projecting calls refuse the model
  7  the host route: lfvio_host_track_trace and lfvio_host_replay_images on a 12-frame rendered recording with `expand` on write, byte for
     byte, the files they write for the same recording pre-expanded through Engine.remap_apply and tracked with a model-6 camera"""
import os

import numpy as np
import pytest

import equirect_ref as er
import fuse_ref as fr
import image_ref as ir
import project_ref as pr
import track_ref as tr
import tracksource_ref as ts
from test_track_batch import sentinels, untouched
from test_tracker_chain import same

pytestmark = pytest.mark.gpu

SW, SH = 161, 123      # the noise sources
FW, FH = 320, 240      # the rendered stream's frames
OUT = ((131, 67), (128, 64))
S = 50
TABLE = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")
SCALARS = ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject")
ERR_ARG = -1


def kw(size):
    return dict(max_count=40, min_distance=6, mask_radius=6, win_size=15, width=size[0], height=size[1])


def odd_step(width, code):
    bpp = ir.BPP[code]
    return width * bpp + 5 + bpp % 2


class Map:
    """A map's recipe and, from numpy, its float maps for one output size."""

    def __init__(self, kind, size, src_size):
        self.size, self.src_size = size, src_size
        W, H = size
        if kind == "equirect":  # through the PAL camera of a src_size image
            self.cam, self.kind, self.M = pr.small(pr.PAL, pr.CAMS["PAL"][1][0] / src_size[0]), pr.MAP_EQUIRECT, None
        else:  # K^-1 of a distortion-free pinhole camera behind a shift of the output pixel: part of the output looks outside the source
            self.cam, self.kind = pr.small(pr.CAMS["EUROC_ND"][0], pr.CAMS["EUROC_ND"][1][0] / src_size[0]), pr.MAP_PERSPECTIVE
            self.M = pr.K_inverse(self.cam) @ np.array([[1.0, 0.0, -20.0], [0.0, 1.0, 70.0], [0.0, 0.0, 1.0]])
        self.x, self.y = pr.build(self.cam, self.kind, W, H, self.M)

    def build(self, e):
        e.remap_build(self.cam, self.kind, self.size[0], self.size[1], self.M, want_maps=False)

    def remap(self, rows, code, step):
        return pr.remap(rows, self.x, self.y, self.src_size[0], self.src_size[1], code, step)

    def level0(self, rows, code, step):
        return ts.level0(rows, self.x, self.y, self.src_size[0], self.src_size[1], code, step)


@pytest.fixture(scope="module")
def maps():
    """Computed once, shared, never changed."""
    out = {(kind, size, (SW, SH)): Map(kind, size, (SW, SH)) for kind in ("equirect", "perspective") for size in OUT}
    out.update({("equirect", size, (FW, FH)): Map("equirect", size, (FW, FH)) for size in OUT})
    return out


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """Six 320 x 240 frames of the rendered stream: made once, shared, never changed."""
    from lfvio import trace

    p = str(tmp_path_factory.mktemp("tracksource") / "s.lfvt")
    made = trace.make_image_stream(p, seed=2, n_frames=6, scale=4)
    assert (made["width"], made["height"]) == (FW, FH)
    return [img for _, img in trace.read_trace(p)["raw_images"]]


@pytest.fixture(scope="module")
def twin():
    from lfvio.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def words(k):
    return np.random.default_rng([k, 9]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def plain(e, clahe=False):
    """The tracker's state of a fresh context."""
    e.track_frame_reset()
    e.gft_set_mask(None)
    e.clahe_set(3.0, (8, 8)) if clahe else e.clahe_set(None)
    e.image_format(None)
    e.track_source(None)


def arm(e, m, code, step, clahe=False):
    """The setting on: the source image goes up."""
    plain(e, clahe)
    m.build(e)
    e.image_format(code, step)
    e.track_source(*m.src_size)


def arm_chain(e, m, code, clahe=False):
    """The second context of the contract: it is fed lfvio_remap_apply's output under {the same encoding, step 0}."""
    plain(e, clahe)
    m.build(e)
    e.image_format(code, 0)


def expanded(e, m, rows, code, step):
    return e.remap_apply(rows, m.src_size[0], m.src_size[1], m.size, encoding=code, step=step)


def everything(r):
    rj, dt = r["reject"], r["detect"]
    parts = [np.ascontiguousarray(r[key]).tobytes() for key in TABLE]
    parts.append(b"-" if "rows" not in r else np.ascontiguousarray(r["rows"]).tobytes())
    parts.append(repr([r[key] for key in SCALARS] + [r.get("num_rows"), r["rc"], rj["status"], rj["best_sample"], rj["num_inliers"], dt["num_kept"],
                                                     dt["num_corners"], dt["num_candidates"]]).encode())
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
        out.append(px.tobytes())
    return out


def last_error(e):
    return e.lib.lfvio_last_error(e.ctx).decode()


# ---- 1
@pytest.mark.parametrize("size", OUT)
@pytest.mark.parametrize("kind", ("equirect", "perspective"))
def test_level0(eng, maps, kind, size):
    m = maps[kind, size, (SW, SH)]
    W, H = size
    for code in (ir.MONO8, ir.BGR8, ir.RGB8, ir.BGRA8, ir.MONO16, ir.MONO16_BE):
        step = odd_step(SW, code)
        assert step % 2 == 1
        off = pr.offsets(m.x, m.y, SW, SH, step, ir.BPP[code])
        assert (off >= 0).sum() > 0 and (off < 0).sum() > 0  # the gather path and the select path both run
        rows = pr.noise_image(20 + code, SW, SH, code, step)
        arm(eng, m, code, step)
        r = eng.klt_track(rows, np.zeros((0, 2), np.float32), win_size=11, size=size)
        got, want = eng.klt_level(0), m.level0(rows, code, step)
        assert r["rc"] == 0 and got.shape == (H, W) and same(got, want), (kind, size, code)
        assert want[off >= 0].any() and not want[off < 0].any()
    plain(eng)
    eng.remap_reset()


# ---- 2
def run(e, route, imgs, size, cam, pts=None):
    """-> per frame (everything that came back, the pyramid), and the last call's dict"""
    out, r = [], None
    for k, img in enumerate(imgs):
        if route == "klt":
            p = np.zeros((0, 2), np.float32) if k == 0 else pts
            r = e.klt_track(img, p, win_size=11, size=size)
            back = [r["next"].tobytes(), r["status"].tobytes(), r["iterations"].tobytes(), repr((r["levels_used"], r["num_tracked"], r["rc"]))]
            if k == 0:  # the points the later frames track: corners of the first expanded image, by the same call on either context
                pts = e.gft_detect(None, None, max_count=30, min_distance=5, mask_radius=5)["corners"].copy()
                back.append(pts.tobytes())
        else:
            call = e.track_frame_message if route == "message" else e.track_frame
            r = call(img, 5.0 + 0.1 * k, cam, publish=True, words=words(k), stages=True, **kw(size))
            back = everything(r)
        out.append((back, levels(e)))
    return out, r, pts


@pytest.mark.parametrize("clahe", [False, True])
@pytest.mark.parametrize("route,code,size", [("message", ir.BGR8, (131, 67)), ("frame", ir.MONO16, (128, 64)), ("klt", ir.MONO8, (131, 67))])
def test_chain_equality(eng, twin, frames, maps, route, code, size, clahe):
    m = maps["equirect", size, (FW, FH)]
    cam, step = er.camera(*size), odd_step(FW, code)
    rows = [ir.from_gray(g, code, step, seed=30 + k) for k, g in enumerate(frames)]
    assert len(rows) == 6
    arm(eng, m, code, step, clahe)
    arm_chain(twin, m, code, clahe)
    fed = [expanded(twin, m, r, code, step) for r in rows]
    assert all(same(f, m.remap(r, code, step)) for f, r in zip(fed, rows))
    got, last, pts = run(eng, route, rows, size, cam)
    want, _, _ = run(twin, route, fed, size, cam)
    for k in range(6):
        assert got[k][0] == want[k][0], (route, k)
        assert got[k][1] == want[k][1] and len(got[k][1]) >= 2, (route, k)
    if not clahe:  # level 0 is the grey image of the expanded one
        assert got[5][1][0] == m.level0(rows[5], code, step).tobytes()
    if route == "klt":
        print(f"klt: {len(pts)} points, {last['num_tracked']} tracked")
        assert len(pts) >= 10 and last["num_tracked"] >= 5
    else:
        print(f"{route}: {last['num_points']} points, {last['num_tracked']} tracked, {last['num_after_reject']} after rejectWithF")
        assert last["num_points"] >= 10 and last["num_tracked"] >= 5 and last["velocity_3d"].any()
    plain(eng), plain(twin)


# ---- 3
def test_integer_map_owner(eng, twin, frames, maps):
    size = (128, 64)
    m = maps["equirect", size, (FW, FH)]
    cam, code = er.camera(*size), ir.BGR8
    steps = [odd_step(FW, code), 3 * FW, 3 * FW + 8, odd_step(FW, code), 3 * FW + 8, 3 * FW]
    rows = [ir.from_gray(g, code, st, seed=50 + k) for k, (g, st) in enumerate(zip(frames, steps))]
    other = pr.noise_image(77, SW, SH, ir.MONO16, 2 * SW + 3)
    P = np.random.default_rng(5).normal(size=(64, 3)).astype(np.float32) * 4.0
    cloud = fr.pack_cloud(P, 12, (0, 4, 8), big_endian=0, seed=64)
    arm(eng, m, code, steps[0])
    arm_chain(twin, m, code)
    got, want = [], []
    for k in range(6):
        eng.image_format(code, steps[k])
        # the integer map is written for another source between every two frames
        o = eng.remap_apply(other, SW, SH, size, encoding=ir.MONO16, step=2 * SW + 3)
        assert same(o, pr.remap(other, m.x, m.y, SW, SH, ir.MONO16, 2 * SW + 3)), k
        if k % 2:
            f = eng.cloud_fuse(cloud, len(P), 12, (0, 4, 8), size[0], size[1], image=rows[k], image_mode=2, src_size=(FW, FH), encoding=code, step=steps[k],
                               want=("image_out",))
            assert same(f["image_out"], m.remap(rows[k], code, steps[k])), k
            if k == 3:  # ... and for the tracker's own geometry again, then for another
                assert same(eng.remap_apply(other, SW, SH, size, encoding=ir.MONO8, step=SW + 2), pr.remap(other, m.x, m.y, SW, SH, ir.MONO8, SW + 2))
        got.append((everything(eng.track_frame_message(rows[k], 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))), levels(eng)))
        want.append((everything(twin.track_frame_message(expanded(twin, m, rows[k], code, steps[k]), 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))),
                     levels(twin)))
        assert got[k] == want[k], k
        # the apply behind a tracker frame finds the map written for the tracker's source and rebuilds it
        assert same(eng.remap_apply(other, SW, SH, size, encoding=ir.MONO16, step=2 * SW + 3), pr.remap(other, m.x, m.y, SW, SH, ir.MONO16, 2 * SW + 3)), k
    plain(eng), plain(twin)


# ---- 4
def refused(e, img, size, cam, why, level0):
    """Both kinds of call are refused with a message; pre-filled outputs and the resident image stay."""
    from lfvio import abi

    nxt, stat = np.full((4, 2), 7.5, np.float32), np.full(4, 77, np.uint8)
    r = e.klt_track(img, np.full((4, 2), 20.0, np.float32), next=nxt, status=stat, size=size, check=False)
    assert r["rc"] == ERR_ARG and why in last_error(e) and (nxt == 7.5).all() and (stat == 77).all(), (why, last_error(e))
    bufs = sentinels(1)
    arrays, o, rows_out = bufs[0]
    for message in (True, False):
        msg = abi.TrackMessageC()
        msg.num_rows = -77
        if message:
            r = e.track_frame_message(img, 9.0, cam, publish=True, words=words(0), out=o, arrays=arrays, rows=rows_out, msg=msg, check=False, **kw(size))
        else:
            r = e.track_frame(img, 9.0, cam, publish=True, words=words(0), out=o, arrays=arrays, check=False, **kw(size))
        assert r["rc"] == ERR_ARG and why in last_error(e) and untouched(bufs, [dict(msg_num_rows=int(msg.num_rows))]), (why, last_error(e))
    got = e.klt_level(0, check=False)
    assert (got is None and level0 is None) or same(got, level0), why


def test_refusals(eng, twin, frames, maps):
    from lfvio.engine import Engine

    size, code = (131, 67), ir.BGR8
    m, wrong = maps["equirect", size, (FW, FH)], maps["equirect", (128, 64), (FW, FH)]
    cam, step = er.camera(*size), odd_step(FW, code)
    rows = [ir.from_gray(g, code, step, seed=70 + k) for k, g in enumerate(frames[:3])]
    # the context that never sees a refused call
    arm(twin, m, code, step)
    want = [(everything(twin.track_frame_message(r, 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))), levels(twin)) for k, r in enumerate(rows)]
    # no map: a context that never built one
    fresh = Engine(0)
    try:
        fresh.image_format(code, step)
        fresh.track_source(FW, FH)
        refused(fresh, rows[0], size, cam, "no resident map", None)
        m.build(fresh)
        r = fresh.track_frame_message(rows[0], 5.0, cam, publish=True, words=words(0), **kw(size))
        assert (everything(r), levels(fresh)) == want[0]
    finally:
        fresh.close()
    # the others between the frames of one stream
    arm(eng, m, code, step)
    for side in (15, 8193):  # the set call refuses; the setting stays
        assert eng.track_source(side, FH, check=False) == ERR_ARG and "[16, 8192]" in last_error(eng)
        assert eng.track_source(FW, side, check=False) == ERR_ARG and "[16, 8192]" in last_error(eng)
    assert eng.lib.lfvio_track_source_set(None, None) == ERR_ARG
    r = eng.track_frame_message(rows[0], 5.0, cam, publish=True, words=words(0), **kw(size))
    assert (everything(r), levels(eng)) == want[0]
    level0 = eng.klt_level(0)
    wrong.build(eng)
    refused(eng, rows[1], size, cam, "another size", level0)
    m.build(eng)
    eng.image_format(code, 3 * FW - 1)  # enough for the 131 pixels tracked, not for the 320 of the source
    assert 3 * FW - 1 > 3 * size[0]
    refused(eng, rows[1], size, cam, "step below width", level0)
    eng.image_format(code, step)
    eng.remap_reset()  # the setting survives, the map does not
    refused(eng, rows[1], size, cam, "no resident map", level0)
    m.build(eng)
    for k in (1, 2):
        r = eng.track_frame_message(rows[k], 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))
        assert (everything(r), levels(eng)) == want[k], k
    assert r["num_points"] >= 10
    plain(eng), plain(twin)


# ---- 5
def test_off_again(eng, twin, frames, maps):
    size = (FW, FH)
    m = maps["equirect", (128, 64), (FW, FH)]
    from lfvio import trace

    cam = trace.image_camera(4)[0]
    arm(eng, m, ir.MONO8, 0)
    eng.klt_track(frames[0], np.zeros((0, 2), np.float32), size=m.size)
    assert eng.klt_level(0).shape == (64, 128)
    eng.track_source(None)
    eng.track_frame_reset()
    plain(twin)
    twin.remap_reset()
    for k, g in enumerate(frames[:3]):
        a = eng.track_frame_message(g, 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))
        b = twin.track_frame_message(g, 5.0 + 0.1 * k, cam, publish=True, words=words(k), **kw(size))
        assert everything(a) == everything(b) and levels(eng) == levels(twin), k
    assert same(eng.klt_level(0), frames[2]) and a["num_points"] >= 10
    plain(eng)
    eng.remap_reset()


# ---- 6
@pytest.mark.parametrize("N", (37, 200))
def test_lift_on_the_device(eng, N):
    cam = er.camera(960, 480)
    cur, forw = er.make_matches(N, cam, N)
    samples = tr.make_samples(3, N, 100)
    want = er.reject(cam, cur, forw, samples)
    got = eng.track_reject(cam, cur, forw, samples, want_bearings=True)
    assert same(got["bearing_cur"], want["bearing_cur"]) and same(got["bearing_forw"], want["bearing_forw"])
    assert got["status"] == want["status"] == 0 and same(got["mask"], want["mask"])
    assert (got["best_sample"], got["num_inliers"]) == (want["best_sample"], want["num_inliers"]) and 8 <= got["num_inliers"] < N
    # E and the score: numpy's E comes out of LAPACK's SVD and is nobody's bits (tests/test_track.py compares it for no model); the
    # device's own two-view path on the restatement's bearings is, as for every other model
    t = eng.two_view(want["bearing_cur"], want["bearing_forw"], samples)
    assert same(got["E"], np.asarray(t["E"], np.float64).reshape(9)) and np.float64(got["best_score"]).tobytes() == np.float64(t["best_score"]).tobytes()
    eng.track_reset()
    ref, ids = er.Undistort(), np.arange(N, dtype=np.int32)
    ids[::7] = -1
    for k, pts in enumerate((cur, forw, cur)):
        w = ref(cam, pts, ids, 1.0 + 0.1 * k)
        g = eng.track_undistort(cam, pts, ids, 1.0 + 0.1 * k)
        for key in ("un_pts", "un_pts_3d", "velocity_3d", "matched"):
            assert same(g[key], w[key]), (k, key)
    assert g["velocity_3d"].any()
    eng.track_reset()
    # the lift only: every projecting call refuses the model, with a message of its own
    rc, _ = eng.cam_project(cam, np.array([[0.1, 0.2, 1.0]]), check=False)
    assert rc == ERR_ARG and "lift only" in last_error(eng)
    assert eng.remap_build(cam, pr.MAP_EQUIRECT, 33, 17, check=False)[0] == ERR_ARG and "lift only" in last_error(eng)
    cloud = fr.pack_cloud(np.ones((4, 3), np.float32), 12, (0, 4, 8), big_endian=0, seed=4)
    rc, _ = eng.cloud_fuse(cloud, 4, 12, (0, 4, 8), 33, 17, kind=1, cam=cam, check=False)
    assert rc == ERR_ARG and "lift only" in last_error(eng)
    for bad in (er.camera(15, 480), er.camera(960, 8193), er.camera(960.5, 480), er.camera(float("nan"), 480)):
        assert eng.track_undistort(bad, cur, ids, 1.0, check=False)["rc"] == ERR_ARG and "EQUIRECT" in last_error(eng)


def test_batch_slot_with_the_equirect_camera(eng, frames, maps):
    from lfvio.engine import Engine

    size = (131, 67)
    m = maps["equirect", size, (FW, FH)]
    cam = er.camera(*size)
    imgs = [m.level0(g, ir.MONO8, 0) for g in frames[:3]]  # the expanded grey images, from numpy: the batch takes the tracked image
    entries = [dict(img=g, time=7.0 + 0.1 * k, cam=cam, words=words(k)) for k, g in enumerate(imgs)]
    try:
        eng.track_batch_reserve(1)
        eng.track_batch_clahe(None)
        eng.track_batch_format(None)
        eng.track_source(FW, FH)  # the batched route does not look at the setting
        got = [eng.track_batch_frame([f], **kw(size))[0] for f in entries]
    finally:
        eng.track_source(None)
        eng.track_batch_reserve(0)
    alone = Engine(0)
    try:
        want = [alone.track_frame_message(f["img"], f["time"], cam, publish=True, words=f["words"], **kw(size)) for f in entries]
    finally:
        alone.close()
    for k in range(3):
        assert everything(got[k]) == everything(want[k]), k
    assert got[2]["num_points"] >= 10 and got[2]["velocity_3d"].any()


# ---- 7
def pre_expanded(eng, src, dst, m):
    """The recording `src` (mono8 records of m.src_size) with every image replaced by its expanded one, through Engine.remap_apply."""
    import struct

    body = open(src, "rb").read()
    out, o, k = [body[:8]], 8, 0
    while o < len(body):
        kind, n = struct.unpack_from("<II", body, o)
        p = body[o + 8:o + 8 + n]
        o += 8 + n
        if kind == 10:
            t, w, h, step, enc = struct.unpack("<dIIII", p[:24])
            assert (w, h, enc) == (m.src_size[0], m.src_size[1], 0)
            rows = np.frombuffer(p[24:], np.uint8).reshape(h, step)
            big = eng.remap_apply(rows, w, h, m.size, encoding=ir.MONO8, step=step)
            assert big.shape == (m.size[1], m.size[0])
            p = struct.pack("<dIIII", t, m.size[0], m.size[1], m.size[0], 0) + big.tobytes()
            k += 1
        out.append(struct.pack("<II", kind, len(p)) + p)
    open(dst, "wb").write(b"".join(out))
    return k


def test_host_route(eng, tmp_path):
    """lfvio_host_track_trace and lfvio_host_replay_images with `expand` on against the same recording pre-expanded and tracked with the
    model-6 camera and `expand` off: the same files, byte for byte."""
    from lfvio import trace
    from lfvio.host import HostEstimator

    src, pre = str(tmp_path / "raw.lfvt"), str(tmp_path / "expanded.lfvt")
    made = trace.make_image_stream(src, seed=0, n_frames=12, scale=4)
    assert (made["width"], made["height"]) == (FW, FH)
    m = Map("equirect", (320, 160), (FW, FH))
    m.build(eng)
    assert pre_expanded(eng, src, pre, m) == 12
    eng.remap_reset()
    cam, out = er.camera(*m.size), {}
    for expand, path in ((True, src), (False, pre)):
        he = HostEstimator()  # a fresh estimator and context for either route
        try:
            he.clear_state()
            he.set_min_parallax(10.0)
            he.set_solver_time(0.0)
            he.track_config(cam, max_cnt=80, min_dist=12, freq=10, num_samples=100, seed=77)
            if expand:
                he.track_expand(m.cam, m.kind, m.size[0], m.size[1])
            tracked, traj = str(tmp_path / f"tracked{int(expand)}.lfvt"), str(tmp_path / f"traj{int(expand)}.txt")
            rc0, ts0 = he.track_trace(path, tracked)
            rc, st, ts = he.replay_images(path, traj)
            strip = lambda d: {k: v for k, v in d.items() if k != "tracker_ms"}
            out[expand] = (rc0, strip(ts0), open(tracked, "rb").read(), rc, st, strip(ts), open(traj, "rb").read() if os.path.exists(traj) else None)
        finally:
            he.close()
    assert out[True] == out[False]
    rc0, ts0, tracked = out[True][:3]
    print(f"host route: {ts0}")
    assert rc0 == 0 and ts0["raw_images"] == 12 and ts0["published"] >= 9 and ts0["rows"] >= 9 * 20 and len(tracked) > 0
