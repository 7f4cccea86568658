"""The KANNALA_BRANDT camera model on the device (kb_lift_pixel behind cam_lift, camera_models.h over camera_kb.h) through every route that
takes an LfvioCamera, bit for bit unless said, against tests/kb_ref.py and against the library's own other routes.  Every test here
fails on a library that answers LFVIO_ERR_ARG for model 5.

  1  the lift: bearing_cur / bearing_forw equal kb_ref.bearings on every fixture case; on 2 x 1031 pixels over and 50 px beyond the
     image for all six cameras, one after the other on one context (2062 threads: nine workgroups, the cur / forw boundary inside
     one; RSFISH reaches the fallback branch, and the context's cached constants have to follow every change of camera); on the NaN,
     +-inf and +-3e38 pixels, NaN positions as a mask and every other value as bytes
  2  the RANSAC against lfvio_two_view on the restatement's bearings: N = 8, 9, 65, 257, S = 4 and 100, the cameras alternating; no
     tolerance, at least four cases find a model.  And against kb_ref.reject on the fixture: mask, best_sample, num_inliers; a case
     that breaks C1 / C2 on the restatement would drop out, at most 10 % may (tests/test_kb_ref.py asserts that none does)
  3  undistortedPoints: the fixture's four-call sequences at N = 40 (every camera) and one of N = 257 (two workgroups) against
     kb_ref.Undistort: un_pts, un_pts_3d, velocity, matched
  4  one frame in one call: six 188 x 120 images of make_image_stream through TUM / (512 / 188) and RSFISH / (640 / 188) — the image
     circle covers the frame — through lfvio_track_frame_message, and through the chain of the separate calls on a second context:
     the table, every stage and the message rows are equal, and the rejection found a model at least once
  5  batch: four slots with an OCam, a PINHOLE, a MEI and a KANNALA_BRANDT camera behind one launch, four frames, one slot idle in one
     call; each slot equals a fresh context given its frames.  The KANNALA_BRANDT slot changes its camera from TUM to RSFISH / 5
     between the second and the third call (points beyond RSFISH's r_lim among them): the slot's cached constants follow it
  6  arguments: every refused field on lfvio_track_reject; poly[0] = NaN and fx = 0 on the other four routes; outputs filled with
     0x5A stay, and the next good call gives a fresh context's bits
  7  the other models are unchanged: the camera_cases.npz and track_cases.npz bearings with NaN written into poly, c, d, e (PINHOLE,
     MEI) and into fx .. xi (OCam)
  8  the host tracker (lfvio_host_track_trace) over test 4's recording with the KANNALA_BRANDT camera configured: its messages equal
     the single-call route's as the node gates them, row for row"""
import ctypes as C
import os

import numpy as np
import pytest

import camera_ref as cr
import kb_ref as kb
import node_ref as nr
import track_frame_ref as tf
import track_ref as tr
from test_camera_models import (H, KEYS4, KW, MAX_CNT, MIN_DIST, NAN, S, SCALE, SEED, W, MessageEngine, filled, frame_buffers, record, same, single,
                                slot_words, untouched, words)
from test_kb_ref import same_but_nan, special_pixels, wide_pixels

pytestmark = pytest.mark.gpu

TUM_S, RSFISH_S = kb.scaled(kb.TUM, 512 / W), kb.scaled(kb.RSFISH, 640 / W)
RSFISH_5 = kb.scaled(kb.RSFISH, 5)  # on a 188 x 120 image: r > r_lim right of x = 151


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "kb_cases.npz"))
    return {k: z[k] for k in z.files}


def fixture_case(fx, name):
    return kb.cam_from_vector(fx[f"{name}/cam"]), fx[f"{name}/cur"], fx[f"{name}/forw"], fx[f"{name}/samples"]


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    """name -> dict(path, camera, images, stamps): six 188 x 120 images each.  TUM, RSFISH, EUROC, MV3DM: make_image_stream through the
    scaled camera.  OCAM: the 320 x 240 stream of trace.image_camera(4) cut to the same size (tests/test_camera_models.py).  Made once,
    shared, never changed."""
    from lfvio import trace

    d = tmp_path_factory.mktemp("kb_streams")
    out = {}
    for name, cam in (("TUM", TUM_S), ("RSFISH", RSFISH_S), ("EUROC", cr.scaled(cr.EUROC, SCALE)), ("MV3DM", cr.scaled(cr.MV3DM, SCALE))):
        p = str(d / f"{name}.lfvt")
        made = trace.make_image_stream(p, seed=2, n_frames=6, camera=(cam, W, H))
        raw = trace.read_trace(p)["raw_images"]
        assert [t for t, _ in raw] == made["stamps"] and raw[0][1].shape == (H, W) and np.all(made["mask"] == 255)
        out[name] = dict(path=p, camera=cam, images=[img for _, img in raw], stamps=made["stamps"])
    p = str(d / "OCAM.lfvt")
    made = trace.make_image_stream(p, seed=3, n_frames=6, scale=SCALE)
    cam, (cx, cy, r_out, _) = made["camera"], made["annulus"]
    x0, y0 = int(round(cx)) - W // 2, max(int(round(cy - r_out)) - 4, 0)
    raw = trace.read_trace(p)["raw_images"]
    out["OCAM"] = dict(camera=dict(cam, cx=cam["cx"] - x0, cy=cam["cy"] - y0), stamps=made["stamps"],
                       images=[np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W]) for _, img in raw])
    return out


# ---- 1
def test_lift(eng, fx):
    n = 0
    for name in kb.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if len(cur) < 8:
            continue
        d = eng.track_reject(cam, cur, forw, s, want_bearings=True)
        assert same(d["bearing_cur"], kb.bearings(cam, cur)) and same(d["bearing_forw"], kb.bearings(cam, forw)), name
        assert same(d["bearing_cur"], fx[f"{name}/bearing_cur"]) and same(d["bearing_forw"], fx[f"{name}/bearing_forw"]), name
        n += 1
    assert n >= 7
    fallback = {}
    for name, cam in list(kb.CAMERAS.items()) + [("TUM", kb.TUM)]:  # (and back to the first: the cached constants follow)
        px = wide_pixels(name)
        d = eng.track_reject(cam, px[:1031], px[1031:], tr.make_samples(1, 1031, 1), want_bearings=True)
        assert same(d["bearing_cur"], kb.bearings(cam, px[:1031])) and same(d["bearing_forw"], kb.bearings(cam, px[1031:])), name
        assert np.isfinite(d["bearing_cur"]).all() and np.isfinite(d["bearing_forw"]).all(), name
        fallback[name] = int(kb.fell_back(cam, kb.plane(cam, px)[2]).sum())
    assert fallback["RSFISH"] > 0 and fallback["TUM"] == 0, fallback
    for name, cam in kb.CAMERAS.items():
        sp = special_pixels(cam)
        px = np.concatenate([sp, sp[::-1]])[:64]  # (at least 8 matches: the device runs)
        d = eng.track_reject(cam, px[:32], px[32:], tr.make_samples(1, 32, 1), want_bearings=True)
        for got, want in ((d["bearing_cur"], kb.bearings(cam, px[:32])), (d["bearing_forw"], kb.bearings(cam, px[32:]))):
            assert np.isnan(want).any() and not np.isnan(want).all() and same_but_nan(got, want), name


# ---- 2
def against_two_view(eng, cam, cur, forw, s, tag):
    bl, br = kb.bearings(cam, cur), kb.bearings(cam, forw)
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
    cams, models = list(kb.CAMERAS.values()), 0
    for i, N in enumerate((8, 9, 65, 257)):
        for j, S_ in enumerate((4, 100)):
            cam = cams[(2 * i + j) % len(cams)]
            cur, forw = kb.make_matches(100 + i, cam, N, **kb.small(N))
            models += against_two_view(eng, cam, cur, forw, kb.make_samples(200 + 2 * i + S_, N, S_), f"N={N} S={S_}") == 0
    assert models >= 4


def test_ransac_equals_the_restatement(eng, fx):
    dropped, total = [], 0
    for name in kb.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if int(fx[f"{name}/status"]) != 0:
            continue
        total += 1
        r = kb.reject(cam, cur, forw, s)
        assert same(r["mask"], fx[f"{name}/mask"]), name
        if not kb.conditions(r):
            dropped.append(name)
            continue
        d = eng.track_reject(cam, cur, forw, s)
        assert d["status"] == 0 and d["best_sample"] == r["best_sample"] and d["num_inliers"] == r["num_inliers"], name
        assert same(d["mask"], r["mask"]), name
    assert total >= 7 and len(dropped) <= 0.1 * total, dropped
    cam, cur, forw, s = fixture_case(fx, "cla_7")  # fewer than 8 matches: no device work
    d = eng.track_reject(cam, cur, forw, None, num_samples=0)
    assert (d["status"], d["best_sample"], d["num_inliers"]) == (2, -1, 0) and np.all(d["mask"] == 1)


# ---- 3
def run_sequence(eng, cam, calls):
    state = kb.Undistort()
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
        cam = kb.cam_from_vector(fx[f"{s}/cam"])
        calls = [(fx[f"{s}/{j}/pts"], fx[f"{s}/{j}/ids"], float(fx[f"{s}/{j}/time"])) for j in range(int(fx[f"{s}/calls"]))]
        assert len(calls) == 4 and len(calls[0][0]) == 40
        outs = run_sequence(eng, cam, calls)
        for j, r in enumerate(outs):
            for key in KEYS4:
                assert same(r[key], fx[f"{s}/{j}/{key}"]), (s, j, key)
        assert outs[1]["velocity_3d"].any() and (outs[2]["matched"] >= 0).sum() > 20
    # N = 257: the second workgroup holds one point; every call is passed back to front, so that the point of index 256 is the oldest
    calls = [(pts[::-1], ids[::-1], t) for pts, ids, t in kb.undistort_sequence(31, kb.RSFISH, calls=3, N=257)]
    outs = run_sequence(eng, kb.RSFISH, calls)
    assert len(outs[1]["matched"]) == 257 and outs[1]["matched"][256] >= 0 and outs[2]["matched"][256] >= 0 and outs[2]["velocity_3d"][256].any()


# ---- 4
@pytest.fixture(scope="module")
def singles(eng, streams):
    """Test 4's single-call route per stream: computed once, shared by tests 4, 6 and 8, never changed."""
    return {name: single(eng, streams[name]) for name in ("TUM", "RSFISH")}


@pytest.mark.parametrize("name", ["TUM", "RSFISH"])
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
            assert same(rec["un_pts_3d"], kb.bearings(st["camera"], rec["cur_pts"]).astype(np.float32)), (name, k)
    finally:
        second.close()
    assert ress[0]["num_points"] >= 20 and ress[-1]["num_rows"] >= 8 and ress[-1]["velocity_3d"].any()
    assert sum(r["reject"]["status"] == 0 for r in ress) >= 1  # the rejection did real work
    assert np.isfinite(ress[-1]["un_pts"]).all()


# ---- 5
def test_batch_of_four_models(eng, streams):
    from lfvio.engine import Engine

    names = ("OCAM", "EUROC", "MV3DM", "TUM")
    cols = [[dict(img=streams[n]["images"][k], time=streams[n]["stamps"][k], cam=streams[n]["camera"], publish=True, words=slot_words(slot, k))
             for k in range(4)] for slot, n in enumerate(names)]
    cols[1][2] = None  # the PINHOLE slot is idle in the third call
    for k in (2, 3):
        cols[3][k]["cam"] = RSFISH_5  # the KANNALA_BRANDT slot's camera changes between two calls
    eng.track_batch_reserve(4)
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
    # the KANNALA_BRANDT slot's bearings are the restatement's under the camera of each call, the fallback branch of the new one included
    beyond = 0
    for k in range(4):
        g, cam = got[k][3], cols[3][k]["cam"]
        pts = g["pts"][:g["num_points"]]
        assert same(g["un_pts_3d"][:g["num_points"]], kb.bearings(cam, pts).astype(np.float32)), k
        beyond += int(kb.fell_back(cam, kb.plane(cam, pts)[2]).sum()) if k >= 2 else 0
    assert beyond > 0
    eng.track_batch_reserve(0)


# ---- 6
def refused_cameras():
    out = [(f"model {m}", dict(kb.TUM, model=m)) for m in (1, 4, 7, -1)]
    for tag, base in (("TUM", kb.TUM), ("RSFISH", kb.RSFISH)):
        out += [(f"{tag} {key} {v}", dict(base, **{key: v})) for key in kb.CHECKED for v in (NAN, float("inf"))]
        out += [(f"{tag} {key} 0", dict(base, **{key: 0.0})) for key in ("fx", "fy")]
    return out


def test_arguments(eng, streams, singles):
    from lfvio import abi

    cam = kb.CLA
    cur, forw = kb.make_matches(61, cam, 40)
    s = kb.make_samples(62, 40, 5)
    want = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    bad = refused_cameras()
    assert len(bad) == 4 + 2 * 18
    for tag, c in bad:
        assert kb.common_check(c, 40), tag
        out = abi.TrackRejectOutC()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        mask, bc, bf = filled(40, np.uint8), filled((40, 3), np.float64), filled((40, 3), np.float64)
        d = eng.track_reject(c, cur, forw, s, out=out, status=mask, bearings=(bc, bf), check=False)
        assert d["rc"] == -1, tag  # LFVIO_ERR_ARG
        assert bytes(out) == b"\x5a" * C.sizeof(out) and untouched(mask, bc, bf), tag
    for c in (dict(kb.CLA, fx=-472.3), kb.KB_IDEAL, dict(kb.CLA, k1=NAN, k2=3.0, xi=NAN, c=NAN)):  # accepted: what the model does not read
        assert not kb.common_check(c, 40) and eng.track_reject(c, cur, forw, s, check=False)["rc"] == 0
    got = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    assert all(same(got[k], want[k]) for k in ("mask", "E", "bearing_cur", "bearing_forw")) and got["status"] == want["status"] == 0

    two = (("poly[0] NaN", dict(kb.TUM, k2=NAN)), ("fx 0", dict(kb.TUM, fx=0.0)))
    # lfvio_track_undistort: the outputs, the resident map and the time
    seq = kb.undistort_sequence(63, cam, calls=2, N=30)
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
    st, ref = streams["TUM"], singles["TUM"]
    single(eng, st, frames=range(2))
    for tag, c in two:
        cs = kb.scaled(c, 512 / W)
        for message in (False, True):
            arrays, out, rows = frame_buffers()
            head = bytes(out)[:abi.TrackFrameOutC.pts.offset]
            if message:
                msg = abi.TrackMessageC()
                msg.num_rows = -77
                r = eng.track_frame_message(st["images"][2], st["stamps"][2], cs, rows=rows, msg=msg, words=words(2), arrays=arrays, out=out, check=False, **KW)
                assert msg.num_rows == -77, tag
            else:
                r = eng.track_frame(st["images"][2], st["stamps"][2], cs, words=words(2), arrays=arrays, out=out, check=False, **KW)
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
        res = eng.track_batch_frame([entry(2, st["camera"]), entry(2, kb.scaled(c, 512 / W))], buffers=bufs, check=False, **KW)
        assert res[0]["rc"] == -1, tag
        for i, (arrays, out, rows) in enumerate(bufs):
            assert bytes(out)[:len(heads[i])] == heads[i] and untouched(rows, *arrays.values()) and res[i]["msg_num_rows"] == -77, (tag, i)
    res = eng.track_batch_frame([entry(2, st["camera"]), entry(2, st["camera"])], **KW)
    assert record(res[0]) == record(ref[2]) and record(res[1]) == record(ref[2])
    eng.track_batch_reserve(0)


# ---- 7
def test_the_other_models_are_unchanged(eng, golden_dir):
    z = np.load(os.path.join(golden_dir, "camera_cases.npz"))
    unread = dict(c=NAN, d=NAN, e=NAN, poly=(NAN,) * 5)
    n = 0
    for name in cr.CASES:
        cam = dict(cr.cam_from_vector(z[f"{name}/cam"]), **unread)
        cur, forw, s = z[f"{name}/cur"], z[f"{name}/forw"], z[f"{name}/samples"]
        if len(cur) < 8:
            continue
        assert np.isnan(eng.camera(cam).poly[0]) and np.isnan(eng.camera(cam).c)
        d = eng.track_reject(cam, cur, forw, s, want_bearings=True)
        assert same(d["bearing_cur"], z[f"{name}/bearing_cur"]) and same(d["bearing_forw"], z[f"{name}/bearing_forw"]) and same(d["mask"], z[f"{name}/mask"]), name
        n += 1
    assert n >= 6
    z = np.load(os.path.join(golden_dir, "track_cases.npz"))
    new = dict(fx=NAN, fy=NAN, k1=NAN, k2=NAN, p1=NAN, p2=NAN, xi=NAN)
    n = 0
    for name in tr.CASES:
        cam = dict(tr.cam_from_vector(z[f"{name}/cam"]), **new)
        cur, forw, s = z[f"{name}/cur"], z[f"{name}/forw"], z[f"{name}/samples"]
        if len(cur) < 8:
            continue
        d = eng.track_reject(cam, cur, forw, s, want_bearings=True)
        assert same(d["mask"], z[f"{name}/mask"]), name
        if d["status"] != 2:
            assert same(d["bearing_cur"], z[f"{name}/bearing_cur"]) and same(d["bearing_forw"], z[f"{name}/bearing_forw"]), name
            n += 1
    assert n >= 5


# ---- 8
def test_host_tracker_with_a_kannala_brandt_camera(eng, streams, tmp_path):
    from lfvio import trace
    from lfvio.host import HostEstimator

    st = streams["TUM"]
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
