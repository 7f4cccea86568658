"""The PINHOLE and MEI camera models on the device (cam_lift_pinhole / cam_lift_mei behind cam_lift, camera_models.h) through every route
that takes an LfvioCamera, bit for bit unless said, against tests/camera_ref.py and against the library's own other routes.

  1  the lift: bearing_cur / bearing_forw equal camera_ref.bearings on every fixture case and on 2 x 1031 pixels over and 50 px beyond
     the 752 x 480 image, for every camera; NaNs are compared as bits
  2  the RANSAC against lfvio_two_view on the restatement's bearings: N = 8, 9, 65, 257, S = 4 and 100, the cameras alternating; no
     tolerance, no case dropped, at least four cases find a model
  3  the RANSAC against the restatement on the fixture cases: mask, best_sample, num_inliers; a case that breaks C1 / C2 on the
     restatement would drop out, at most 10 % may (tests/test_camera_ref.py asserts that none does)
  4  undistortedPoints: the fixture's sequences (four calls, N = 40, every camera) and one of N = 257 (two workgroups) against
     camera_ref.Undistort
  5  one frame in one call: six images of a 188 x 120 make_image_stream through EUROC / 4 (and MV3DM / 4) through
     lfvio_track_frame_message, and through the chain of the separate calls on a second context: the table, the outputs of
     undistortedPoints, the message rows, reject, detect and every stage are equal, and the rejection found a model at least once
  6  batch: three slots with an OCam, a PINHOLE and a MEI camera behind one launch, four frames, one slot idle in one call; each slot
     equals a fresh context given its frames
  7  arguments: every refused camera field on lfvio_track_reject, model 1 and fx = 0 on the other four routes; outputs filled with
     0x5A stay, and the next good call gives the bits of a fresh context
  8  OCam unchanged: an OCam camera with NaN in every new field gives the bits of tests/golden/track_cases.npz
  9  the host tracker (lfvio_host_track_trace) over test 5's six-image recording with the PINHOLE camera configured: its feature
     messages equal the single-call route's as the node gates it (image 0 dropped, the first publication skipped, the words
     std::mt19937's), row for row"""
import ctypes as C
import os

import numpy as np
import pytest

import camera_ref as cr
import node_ref as nr
import track_frame_ref as tf
import track_ref as tr

pytestmark = pytest.mark.gpu

S = 100
W, H, SCALE = 188, 120, 4
MAX_CNT, MIN_DIST = 40, 10
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
TABLE = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")
SCALARS = ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject", "num_rows")
EUROC4, MV3DM4 = cr.scaled(cr.EUROC, SCALE), cr.scaled(cr.MV3DM, SCALE)
NAN = float("nan")
SEED = 20240611


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "camera_cases.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ocam_fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "track_cases.npz"))
    return {k: z[k] for k in z.files}


def fixture_case(fx, name):
    return cr.cam_from_vector(fx[f"{name}/cam"]), fx[f"{name}/cur"], fx[f"{name}/forw"], fx[f"{name}/samples"]


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    """name -> dict(path, camera, images, stamps): six 188 x 120 images each.  PINHOLE and MEI: make_image_stream through the scaled
    camera.  OCAM: the 320 x 240 stream of trace.image_camera(4) cut to the same size around the upper part of its annulus, the
    camera's centre moved by the cut's corner.  Made once, shared, never changed."""
    from lfvio import trace

    d = tmp_path_factory.mktemp("camera_streams")
    out = {}
    for name, cam in (("EUROC", EUROC4), ("MV3DM", MV3DM4)):
        p = str(d / f"{name}.lfvt")
        made = trace.make_image_stream(p, seed=2, n_frames=6, camera=(cam, W, H))
        raw = trace.read_trace(p)["raw_images"]
        assert [t for t, _ in raw] == made["stamps"] and raw[0][1].shape == (H, W)
        out[name] = dict(path=p, camera=cam, images=[img for _, img in raw], stamps=made["stamps"], mask=made["mask"])
    p = str(d / "OCAM.lfvt")
    made = trace.make_image_stream(p, seed=3, n_frames=6, scale=SCALE)
    cam, (cx, cy, r_out, _) = made["camera"], made["annulus"]
    x0, y0 = int(round(cx)) - W // 2, max(int(round(cy - r_out)) - 4, 0)
    raw = trace.read_trace(p)["raw_images"]
    out["OCAM"] = dict(camera=dict(cam, cx=cam["cx"] - x0, cy=cam["cy"] - y0), stamps=made["stamps"],
                       images=[np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W]) for _, img in raw])
    assert out["OCAM"]["images"][0].shape == (H, W) and (out["OCAM"]["images"][0] > 0).mean() > 0.3
    return out


# ---- 1
def test_lift(eng, fx):
    n = 0
    for name in cr.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if len(cur) < 8:
            continue
        d = eng.track_reject(cam, cur, forw, s, want_bearings=True)
        assert same(d["bearing_cur"], cr.bearings(cam, cur)) and same(d["bearing_forw"], cr.bearings(cam, forw)), name
        assert same(d["bearing_cur"], fx[f"{name}/bearing_cur"]) and same(d["bearing_forw"], fx[f"{name}/bearing_forw"]), name
        n += 1
    assert n >= 6
    rng = np.random.default_rng(8)
    px = rng.uniform([-50.0, -50.0], [cr.WIDTH + 50.0, cr.HEIGHT + 50.0], (2 * 1031, 2)).astype(np.float32)
    for name, cam in cr.CAMERAS.items():
        d = eng.track_reject(cam, px[:1031], px[1031:], tr.make_samples(1, 1031, 1), want_bearings=True)
        assert same(d["bearing_cur"], cr.bearings(cam, px[:1031])) and same(d["bearing_forw"], cr.bearings(cam, px[1031:])), name
        assert np.isfinite(d["bearing_cur"]).all(), name  # (the five cameras are finite that close to the image)
    # beyond what the five cameras reach: a short focal length, so that the MEI root goes negative inside the drawn pixels.  The
    # same points are NaN on both sides and every other value has the same bits.  The NaNs' own bits are not compared HERE: IEEE 754
    # leaves the sign and payload of a NaN that an invalid operation makes to the implementation, and the two differ (measured:
    # numpy on x86 gives the negative quiet NaN, gfx950 the positive one)
    tiny = dict(cr.MV3DM_ND, fx=300.0, fy=300.0)
    d = eng.track_reject(tiny, px[:1031], px[1031:], tr.make_samples(1, 1031, 1), want_bearings=True)
    for got, want in ((d["bearing_cur"], cr.bearings(tiny, px[:1031])), (d["bearing_forw"], cr.bearings(tiny, px[1031:]))):
        nan = np.isnan(want)
        assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan) and same(got[~nan], want[~nan])


# ---- 2
def against_two_view(eng, cam, cur, forw, s, tag):
    bl, br = cr.bearings(cam, cur), cr.bearings(cam, forw)
    t = eng.two_view(bl, br, s)
    d = eng.track_reject(cam, cur, forw, s)
    assert (d["status"], d["best_sample"], d["num_inliers"]) == (t["status"], t["best_sample"], t["num_inliers"]), tag
    assert np.float64(d["best_score"]).tobytes() == np.float64(t["best_score"]).tobytes(), tag
    if t["status"] == 0:
        assert same(d["mask"], t["mask"]) and same(d["E"], np.asarray(t["E"], np.float64).reshape(9)), tag
        assert int(d["mask"].sum()) == d["num_inliers"]
    else:
        assert np.all(d["mask"] == 1), tag
    return t["status"]


def test_ransac_equals_the_two_view_path(eng):
    cams, models = list(cr.CAMERAS.values()), 0
    for i, N in enumerate((8, 9, 65, 257)):
        for j, S_ in enumerate((4, 100)):
            cam = cams[(2 * i + j) % len(cams)]
            cur, forw = cr.make_matches(100 + i, cam, N, **cr.small(N))
            models += against_two_view(eng, cam, cur, forw, cr.make_samples(200 + 2 * i + S_, N, S_), f"N={N} S={S_}") == 0
    assert models >= 4


# ---- 3
def test_ransac_equals_the_restatement(eng, fx):
    dropped, total = [], 0
    for name in cr.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if int(fx[f"{name}/status"]) != 0:
            continue
        total += 1
        r = cr.reject(cam, cur, forw, s)
        assert same(r["mask"], fx[f"{name}/mask"]), name
        if not cr.conditions(r):
            dropped.append(name)
            continue
        d = eng.track_reject(cam, cur, forw, s)
        assert d["status"] == 0 and d["best_sample"] == r["best_sample"] and d["num_inliers"] == r["num_inliers"], name
        assert same(d["mask"], r["mask"]), name
    assert total >= 6 and len(dropped) <= 0.1 * total, dropped
    cam, cur, forw, s = fixture_case(fx, "mv3dm_7")  # fewer than 8 matches: no device work
    d = eng.track_reject(cam, cur, forw, None, num_samples=0)
    assert (d["status"], d["best_sample"], d["num_inliers"]) == (2, -1, 0) and np.all(d["mask"] == 1)


# ---- 4
KEYS4 = ("un_pts", "un_pts_3d", "velocity_3d", "matched")


def run_sequence(eng, cam, calls):
    state = cr.Undistort()
    eng.track_reset()
    outs = []
    for k, (pts, ids, time) in enumerate(calls):
        r, d = state(cam, pts, ids, time), eng.track_undistort(cam, pts, ids, time)
        for key in KEYS4:
            assert same(d[key], r[key]), (k, key)
        outs.append(r)
    return outs


def test_undistort(eng, fx):
    for s in fx["sequences"]:
        cam = cr.cam_from_vector(fx[f"{s}/cam"])
        calls = [(fx[f"{s}/{j}/pts"], fx[f"{s}/{j}/ids"], float(fx[f"{s}/{j}/time"])) for j in range(int(fx[f"{s}/calls"]))]
        assert len(calls) == 4 and len(calls[0][0]) == 40
        outs = run_sequence(eng, cam, calls)
        for j, r in enumerate(outs):
            for key in KEYS4:
                assert same(r[key], fx[f"{s}/{j}/{key}"]), (s, j, key)
        assert outs[1]["velocity_3d"].any() and (outs[2]["matched"] >= 0).sum() > 20
    # N = 257: the second workgroup holds one point.  The sequence's new points arrive at the end, so every call is passed back to
    # front: the point of index 256 is then the oldest, found in the map, with a velocity
    calls = [(pts[::-1], ids[::-1], t) for pts, ids, t in cr.undistort_sequence(31, cr.MV3DM, calls=3, N=257)]
    outs = run_sequence(eng, cr.MV3DM, calls)
    assert len(outs[1]["matched"]) == 257 and outs[1]["matched"][256] >= 0 and outs[2]["matched"][256] >= 0 and outs[2]["velocity_3d"][256].any()


# ---- 5
def words(k):
    return np.random.default_rng([k, 43]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def single(eng, st, cam=None, frames=range(6), word_of=words):
    eng.clahe_set(None)
    eng.gft_set_mask(None)
    eng.track_frame_reset()
    return [eng.track_frame_message(st["images"][k], st["stamps"][k], cam or st["camera"], words=word_of(k), stages=True, **KW) for k in frames]


@pytest.fixture(scope="module")
def singles(eng, streams):
    """Test 5's single-call route per stream: computed once, shared by tests 5, 6 and 7, never changed."""
    return {name: single(eng, streams[name]) for name in ("EUROC", "MV3DM")}


@pytest.mark.parametrize("name", ["EUROC", "MV3DM"])
def test_one_frame_in_one_call(singles, streams, name):
    from lfvio.engine import Engine
    from lfvio.tracker import FeatureTracker
    from test_track_frame import Recording, agree

    class WordTracker(FeatureTracker):
        def draw_samples(self, n):
            return tf.draw(self.words, n)

    st, ress = streams[name], singles[name]
    second = Engine(0)
    try:
        rec_eng = Recording(second)
        trk = WordTracker(rec_eng, st["camera"], max_cnt=MAX_CNT, min_dist=MIN_DIST, num_samples=S)
        for k, img in enumerate(st["images"]):
            trk.words = words(k)
            rec = trk.read_image(img, st["stamps"][k], publish=True)
            rec.update(klt_out=rec_eng.klt, gft_out=rec_eng.gft)
            agree(rec, ress[k], (name, k))  # the table, the outputs of step 5, reject, detect, every stage
            rows = nr.rows_from_table(rec["cur_pts"], rec["ids"], rec["track_cnt"], rec["un_pts_3d"], rec["velocity_3d"])
            assert same(ress[k]["rows"], rows) and ress[k]["num_rows"] == len(rows), (name, k)
            # and the chain's lift is the restatement's
            assert same(rec["un_pts_3d"], cr.bearings(st["camera"], rec["cur_pts"]).astype(np.float32)), (name, k)
    finally:
        second.close()
    assert ress[0]["num_points"] >= 20 and ress[-1]["num_rows"] >= 8 and ress[-1]["velocity_3d"].any()
    assert sum(r["reject"]["status"] == 0 for r in ress) >= 1  # the rejection did real work
    assert np.isfinite(ress[-1]["un_pts"]).all()


# ---- 6
def record(r):
    rj, dt = r["reject"], r["detect"]
    parts = [np.ascontiguousarray(r[key]).tobytes() for key in TABLE] + [np.ascontiguousarray(r["rows"]).tobytes()]
    parts.append(repr([r[key] for key in SCALARS] + [rj["status"], rj["best_sample"], rj["num_inliers"], dt["num_kept"], dt["num_corners"],
                                                     dt["num_candidates"]]).encode())
    parts += [np.float64(rj["best_score"]).tobytes(), np.ascontiguousarray(rj["E"]).tobytes(), np.float64(dt["max_response"]).tobytes()]
    return parts


def slot_words(slot, k):
    return np.random.default_rng([k, 43, slot]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def test_batch_of_three_models(eng, streams):
    from lfvio.engine import Engine

    names = ("OCAM", "EUROC", "MV3DM")
    cols = [[dict(img=streams[n]["images"][k], time=streams[n]["stamps"][k], cam=streams[n]["camera"], publish=True, words=slot_words(slot, k))
             for k in range(4)] for slot, n in enumerate(names)]
    cols[1][2] = None  # the PINHOLE slot is idle in the third call
    eng.track_batch_reserve(3)
    eng.track_batch_clahe(None)
    got = [eng.track_batch_frame([col[k] for col in cols], **KW) for k in range(4)]
    for slot, n in enumerate(names):
        e = Engine(0)
        try:
            want = [None if f is None else e.track_frame_message(f["img"], f["time"], f["cam"], publish=True, words=f["words"], **KW) for f in cols[slot]]
        finally:
            e.close()
        for k in range(4):
            g = got[k][slot]
            if want[k] is None:
                assert g["num_points"] == 0 and g["num_rows"] == 0 and g["levels_used"] == 0, (n, k)
                continue
            assert g["rc"] == 0 and want[k]["rc"] == 0 and record(g) == record(want[k]), (n, k)
        assert got[3][slot]["num_points"] >= 10 and got[3][slot]["velocity_3d"].any(), n
    eng.track_batch_reserve(0)


# ---- 7
def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = 0x5A
    return a


def untouched(*arrays):
    return all(np.all(np.ascontiguousarray(a).view(np.uint8) == 0x5A) for a in arrays)


def refused_cameras():
    out = [("model 1", dict(cr.EUROC, model=1)), ("model 4", dict(cr.EUROC, model=4)), ("model -1", dict(cr.MV3DM, model=-1))]
    for tag, base in (("PINHOLE", cr.EUROC), ("MEI", cr.MV3DM)):
        out += [(f"{tag} {key} {v}", dict(base, **{key: v})) for key in ("cx", "cy", "fx", "fy", "k1", "k2", "p1", "p2") for v in (NAN, float("inf"))]
        out += [(f"{tag} {key} 0", dict(base, **{key: 0.0})) for key in ("fx", "fy")]
    return out + [("MEI xi nan", dict(cr.MV3DM, xi=NAN)), ("MEI xi inf", dict(cr.MV3DM, xi=-float("inf")))]


def frame_buffers():
    from lfvio import abi

    arrays = dict(pts=filled((4096, 2), np.float32), ids=filled(4096, np.int32), track_cnt=filled(4096, np.int32),
                  un_pts=filled((4096, 2), np.float32), un_pts_3d=filled((4096, 3), np.float32), velocity_3d=filled((4096, 3), np.float32))
    out = abi.TrackFrameOutC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return arrays, out, filled((4096, 9), np.float32)


def test_arguments(eng, streams, singles):
    from lfvio import abi

    cam = cr.EUROC
    cur, forw = cr.make_matches(61, cam, 40)
    s = cr.make_samples(62, 40, 5)
    want = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    bad = refused_cameras()
    assert len(bad) == 3 + 2 * 18 + 2
    for tag, c in bad:
        assert cr.common_check(c, 40), tag
        out = abi.TrackRejectOutC()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        mask, bc, bf = filled(40, np.uint8), filled((40, 3), np.float64), filled((40, 3), np.float64)
        d = eng.track_reject(c, cur, forw, s, out=out, status=mask, bearings=(bc, bf), check=False)
        assert d["rc"] == -1, tag  # LFVIO_ERR_ARG
        assert bytes(out) == b"\x5a" * C.sizeof(out) and untouched(mask, bc, bf), tag
    for c in (dict(cr.EUROC, xi=NAN), dict(cr.EUROC, fx=-461.6), cr.MEI_XI1):  # accepted: PINHOLE does not read xi
        assert not cr.common_check(c, 40) and eng.track_reject(c, cur, forw, s, check=False)["rc"] == 0
    got = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    assert all(same(got[k], want[k]) for k in ("mask", "E", "bearing_cur", "bearing_forw")) and got["status"] == want["status"] == 0

    two = (("model 1", dict(cr.EUROC, model=1)), ("fx 0", dict(cr.EUROC, fx=0.0)))
    # lfvio_track_undistort: the outputs, the resident map and the time
    seq = cr.undistort_sequence(63, cam, calls=2, N=30)
    eng.track_reset()
    eng.track_undistort(cam, *seq[0])
    want_u = eng.track_undistort(cam, *seq[1])
    assert want_u["velocity_3d"].any()
    eng.track_reset()
    eng.track_undistort(cam, *seq[0])
    n = len(seq[1][0])
    for tag, c in two:
        outs = (filled((n, 2), np.float32), filled((n, 3), np.float32), filled((n, 3), np.float32), filled(n, np.int32))
        assert eng.track_undistort(c, seq[1][0], seq[1][1], 9.0, outs=outs, check=False)["rc"] == -1, tag
        assert untouched(*outs), tag
    got_u = eng.track_undistort(cam, *seq[1])
    assert all(same(got_u[k], want_u[k]) for k in KEYS4)

    # lfvio_track_frame and lfvio_track_frame_message: every output, the table, n_id, the resident image, the map and the time
    st, ref = streams["EUROC"], singles["EUROC"]
    single(eng, st, frames=range(2))
    for tag, c in two:
        c4 = cr.scaled(c, SCALE)
        for message in (False, True):
            arrays, out, rows = frame_buffers()
            head = bytes(out)[:abi.TrackFrameOutC.pts.offset]
            if message:
                msg = abi.TrackMessageC()
                msg.num_rows = -77
                r = eng.track_frame_message(st["images"][2], st["stamps"][2], c4, rows=rows, msg=msg, words=words(2), arrays=arrays, out=out, check=False, **KW)
                assert msg.num_rows == -77, tag
            else:
                r = eng.track_frame(st["images"][2], st["stamps"][2], c4, words=words(2), arrays=arrays, out=out, check=False, **KW)
            assert r["rc"] == -1, (tag, message)
            assert bytes(out)[:len(head)] == head and untouched(rows, *arrays.values()), (tag, message)
    got_f = eng.track_frame_message(st["images"][2], st["stamps"][2], st["camera"], words=words(2), stages=True, **KW)
    assert record(got_f) == record(ref[2]) and got_f["velocity_3d"].any()

    # lfvio_track_batch_frame: atomic over the batch, so the good slot beside the refused one is untouched too
    def entry(k, c):
        return dict(img=st["images"][k], time=st["stamps"][k], cam=c, publish=True, words=words(k))

    eng.track_batch_reserve(2)
    eng.track_batch_clahe(None)
    for k in range(2):
        eng.track_batch_frame([entry(k, st["camera"]), entry(k, st["camera"])], **KW)
    for tag, c in two:
        bufs = [frame_buffers(), frame_buffers()]
        heads = [bytes(b[1])[:abi.TrackFrameOutC.pts.offset] for b in bufs]
        res = eng.track_batch_frame([entry(2, st["camera"]), entry(2, cr.scaled(c, SCALE))], buffers=bufs, check=False, **KW)
        assert res[0]["rc"] == -1, tag
        for i, (arrays, out, rows) in enumerate(bufs):
            assert bytes(out)[:len(heads[i])] == heads[i] and untouched(rows, *arrays.values()) and res[i]["msg_num_rows"] == -77, (tag, i)
    res = eng.track_batch_frame([entry(2, st["camera"]), entry(2, st["camera"])], **KW)
    assert record(res[0]) == record(ref[2]) and record(res[1]) == record(ref[2])
    eng.track_batch_reserve(0)


# ---- 8
def test_ocam_is_unchanged(eng, ocam_fx):
    new = dict(fx=NAN, fy=NAN, k1=NAN, k2=NAN, p1=NAN, p2=NAN, xi=NAN)
    n = 0
    for name in tr.CASES:
        cam = dict(tr.cam_from_vector(ocam_fx[f"{name}/cam"]), **new)
        cur, forw, s = ocam_fx[f"{name}/cur"], ocam_fx[f"{name}/forw"], ocam_fx[f"{name}/samples"]
        assert np.isnan(eng.camera(cam).fx) and np.isnan(eng.camera(cam).xi)
        d = eng.track_reject(cam, cur, forw, s if len(cur) >= 8 else None, want_bearings=True, **({} if len(cur) >= 8 else dict(num_samples=0)))
        assert (d["status"], d["best_sample"], d["num_inliers"]) == tuple(int(ocam_fx[f"{name}/{k}"]) for k in ("status", "best_sample", "num_inliers")), name
        assert same(d["mask"], ocam_fx[f"{name}/mask"]), name
        if d["status"] != 2:
            assert same(d["bearing_cur"], ocam_fx[f"{name}/bearing_cur"]) and same(d["bearing_forw"], ocam_fx[f"{name}/bearing_forw"]), name
            n += 1
    assert n >= 5
    for s in ocam_fx["sequences"]:
        cam = dict(tr.cam_from_vector(ocam_fx[f"{s}/cam"]), **new)
        eng.track_reset()
        for j in range(int(ocam_fx[f"{s}/calls"])):
            d = eng.track_undistort(cam, ocam_fx[f"{s}/{j}/pts"], ocam_fx[f"{s}/{j}/ids"], float(ocam_fx[f"{s}/{j}/time"]))
            for key in KEYS4:
                assert same(d[key], ocam_fx[f"{s}/{j}/{key}"]), (s, j, key)


# ---- 9
class MessageEngine:
    """The engine with track_frame routed through lfvio_track_frame_message: node_ref.ImageNode around the single-call route."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def track_frame(self, *a, **kw):
        return self._eng.track_frame_message(*a, **kw)


def test_host_tracker_with_a_pinhole_camera(eng, streams, tmp_path):
    from lfvio import trace
    from lfvio.host import HostEstimator

    st = streams["EUROC"]
    node = nr.ImageNode(MessageEngine(eng), st["camera"], max_cnt=MAX_CNT, min_dist=MIN_DIST, freq=10, num_samples=S, seed=SEED)
    want = [(t,) + node.on_image(t, img) for t, img in zip(st["stamps"], st["images"])]
    kinds = [x[1] for x in want]
    assert kinds == [nr.DROP, nr.FIRST_PUBLICATION] + [nr.PUBLISHED] * 4
    published = [f for f, k in zip(node.frames, kinds[1:]) if k == nr.PUBLISHED]
    msgs = [(t, rows) for t, what, rows in want if what == nr.PUBLISHED]
    for f, (_, rows) in zip(published, msgs):
        assert same(f["rows"], rows)  # the device's message is the table's
    dst = str(tmp_path / "tracked.lfvt")
    he = HostEstimator()
    try:
        he.track_config(st["camera"], max_cnt=MAX_CNT, min_dist=MIN_DIST, freq=10, num_samples=S, seed=SEED)
        rc, ts = he.track_trace(st["path"], dst)
    finally:
        he.close()
    assert rc == 0, rc
    got = trace.read_trace(dst)["images"]
    assert len(got) == len(msgs) == 4
    for k, ((t, rows), (gt, grows)) in enumerate(zip(msgs, got)):
        assert gt == t and same(grows, rows), k
    assert all(len(rows) >= 8 for _, rows in msgs[1:]) and ts["published"] == 4 and ts["dropped"] == 1
