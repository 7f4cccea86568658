"""lfvio_track_frame / lfvio_track_frame_reset on the device against the chain of the separate calls (lfvio.tracker.FeatureTracker on
the same engine), bit for bit, no tolerance and nothing left out.  The images are the klt_ref-rendered 161 x 123 sequence of
tests/test_tracker_chain.py with its settings: MAX_CNT 40, MIN_DIST 10, the scaled PAL camera, S = 100.  The chain draws its sample
sets with track_frame_ref.draw from the words the single call is given.

  1  six frames: the table, the outputs of undistortedPoints, the counts, the rejection record, LfvioGftOut and every stage
  2  the same with publish off on frames 2 and 4
  3  the same with CLAHE (3.0, 8 x 8) on and an annulus base mask
  4  the empty and small cases the host used to filter: a grey first frame, a grey frame after textured ones, max_count = 6 (n1 < 8)
  5  mixing the routes: the separate calls on the table the call returned, and the call again after a reset
  6  every refused field: all outputs untouched, and the next valid frame equals that of a run that never saw the refused calls
  7  repeatability, and frames beside an optimization in flight"""
import ctypes as C

import numpy as np
import pytest

import gft_ref
import track_frame_ref as tf
from test_tracker_chain import CAM, MAX_CNT, MIN_DIST, frames, same

pytestmark = pytest.mark.gpu

S = 100
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
TABLE = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")


@pytest.fixture(scope="module")
def imgs():
    return frames()


def words(k):
    return np.random.default_rng([k, 41]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def when(k):
    return 20.0 + 0.05 * k


class Recording:
    """The engine, keeping what the chain's record drops: LfvioKltOut and LfvioGftOut."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def klt_track(self, *a, **kw):
        self.klt = self._eng.klt_track(*a, **kw)
        return self.klt

    def gft_detect(self, *a, **kw):
        self.gft = self._eng.gft_detect(*a, **kw)
        return self.gft


def chain(eng, images, publish=None, max_cnt=MAX_CNT, first=0):
    """The frames through the separate calls; records as FeatureTracker leaves them plus klt_out and gft_out."""
    from lfvio.tracker import FeatureTracker

    class WordTracker(FeatureTracker):
        def draw_samples(self, n):
            return tf.draw(self.words, n)

    rec_eng = Recording(eng)
    trk = WordTracker(rec_eng, CAM, max_cnt=max_cnt, min_dist=MIN_DIST, num_samples=S)
    out = []
    for k, img in enumerate(images):
        trk.words = words(first + k)
        pub = True if publish is None else publish[k]
        rec = trk.read_image(img, when(first + k), publish=pub)
        rec.update(klt_out=rec_eng.klt, gft_out=rec_eng.gft if pub else None)
        out.append(rec)
    return out, trk


def single(eng, images, publish=None, max_cnt=MAX_CNT, first=0, reset=True):
    if reset:
        eng.track_frame_reset()
    return [eng.track_frame(img, when(first + k), CAM, publish=True if publish is None else publish[k], words=words(first + k), stages=True,
                            **dict(KW, max_count=max_cnt)) for k, img in enumerate(images)]


def agree(rec, res, tag):
    """One frame of the single call against the chain's record."""
    assert same(res["pts"], rec["cur_pts"]), tag
    for key in TABLE[1:]:
        assert same(res[key], rec[key]), (tag, key)
    n1 = int(rec["flow"]["status"].astype(bool).sum())
    assert (res["num_points"], res["num_tracked"], res["levels_used"]) == (len(rec["ids"]), n1, rec["klt_out"]["levels_used"]), tag
    assert res["num_tracked"] == rec["klt_out"]["num_tracked"], tag
    st = res["stages"]
    assert same(st["next"], rec["flow"]["next"]) and same(st["status"], rec["flow"]["status"]), tag
    if not rec["publish"]:
        assert res["num_after_reject"] == n1 and res["num_new"] == 0, tag
        assert res["reject"]["status"] == 0 and res["reject"]["best_score"] == 0.0 and not res["reject"]["E"].any(), tag
        assert res["detect"] == dict(num_kept=0, num_corners=0, num_candidates=0, max_response=0.0), tag
        return
    rj, d = rec["reject"], rec["reject"]["out"]
    got = res["reject"]
    assert (got["status"], got["best_sample"], got["num_inliers"]) == (d["status"], d["best_sample"], d["num_inliers"]), tag
    assert np.float64(got["best_score"]).tobytes() == np.float64(d["best_score"]).tobytes() and same(got["E"], d["E"]), tag
    assert res["num_after_reject"] == int(d["mask"].astype(bool).sum()), tag
    assert same(st["mask"], d["mask"]), tag
    if rj["samples"] is None:
        assert st["samples"] is None and n1 < 8, tag
    else:
        assert same(st["samples"], rj["samples"]), tag
    dt, g = rec["detect"], rec["gft_out"]
    assert same(st["kept"], dt["kept"]) and same(st["corners"], dt["corners"]), tag
    assert res["detect"]["num_kept"] == len(dt["kept"]) and res["detect"]["num_corners"] == len(dt["corners"]), tag
    assert res["detect"]["num_candidates"] == g["num_candidates"], tag
    assert np.float64(res["detect"]["max_response"]).tobytes() == np.float64(g["max_response"]).tobytes(), tag
    assert res["num_new"] == len(dt["corners"]), tag


def both(eng, images, tag, **kw):
    recs, trk = chain(eng, images, **kw)
    ress = single(eng, images, **kw)
    for k, (rec, res) in enumerate(zip(recs, ress)):
        agree(rec, res, (tag, k))
    return recs, ress, trk


def plain(eng):
    eng.clahe_set(None)
    eng.gft_set_mask(None)


def test_six_frames_equal_the_chain(eng, imgs):
    """Test 1."""
    plain(eng)
    recs, ress, trk = both(eng, imgs, "six")
    assert len(recs[0]["ids"]) >= 20 and sum(r["reject"]["out"]["status"] == 0 for r in recs) >= 3
    assert any(r["num_new"] > 0 for r in ress[1:]) and any(r["num_after_reject"] < r["num_tracked"] for r in ress)
    assert sum(r["num_new"] for r in ress) == trk.n_id


def test_without_publish_on_two_frames(eng, imgs):
    """Test 2."""
    plain(eng)
    pub = [k not in (2, 4) for k in range(len(imgs))]
    recs, ress, _ = both(eng, imgs, "publish", publish=pub)
    assert recs[2]["reject"] is None and recs[4]["detect"] is None and ress[2]["num_new"] == 0
    assert ress[2]["num_points"] == ress[2]["num_tracked"] > 8


def test_with_clahe_and_a_base_mask(eng, imgs):
    """Test 3."""
    try:
        eng.klt_reset()
        eng.clahe_set(3.0, (8, 8))
        eng.gft_set_mask(gft_ref.annulus_mask(161, 123, 80, 61, 70, 10))
        recs, ress, _ = both(eng, imgs, "clahe+mask")
        assert len(recs[0]["ids"]) >= 10
        plain(eng)
        unmasked = single(eng, imgs[:1])[0]
        assert not same(unmasked["pts"], ress[0]["pts"])  # the setting and the mask did count
    finally:
        plain(eng)


def test_empty_and_small_cases(eng, imgs):
    """Test 4."""
    plain(eng)
    grey = np.full_like(imgs[0], 117)
    # a grey first frame, then textured ones
    recs, ress, _ = both(eng, [grey, imgs[0], imgs[1], imgs[2]], "grey first")
    assert ress[0]["num_points"] == 0 and ress[0]["detect"]["num_corners"] == 0 and ress[0]["reject"]["status"] == 2
    assert ress[1]["num_points"] >= 20 and ress[1]["num_new"] == ress[1]["num_points"] and not ress[1]["velocity_3d"].any()  # the map was empty
    assert not ress[2]["velocity_3d"].any() and ress[3]["velocity_3d"].any()  # (in the map under -1 a frame ago: the quirk)
    # fewer than 8 matches
    recs, ress, _ = both(eng, imgs[:4], "max_count 6", max_cnt=6)
    for k, r in enumerate(ress):
        assert r["num_tracked"] < 8 and r["reject"]["status"] == 2 and r["num_after_reject"] == r["num_tracked"], k
        assert (r["reject"]["best_sample"], r["reject"]["num_inliers"], r["reject"]["best_score"]) == (-1, 0, 0.0) and r["stages"]["samples"] is None
        assert np.all(r["stages"]["mask"] == 1) and r["num_points"] <= 6
    assert ress[1]["num_tracked"] >= 3
    # grey frames after textured ones.  Into the first some points still "track" (the gradients are the previous image's: measured,
    # 11 of 40 keep status 1) and nothing is detected; from grey into grey every status is 0 (minEig = 0): a table of n0 > 0 entries
    # empties on the device, and the map with it; then it fills again
    recs, ress, _ = both(eng, [imgs[0], imgs[1], grey, grey, imgs[3], imgs[4]], "grey later")
    assert ress[1]["num_points"] >= 20 and ress[2]["detect"]["num_corners"] == 0 and 0 < ress[2]["num_points"] == ress[2]["detect"]["num_kept"]
    assert len(ress[3]["stages"]["status"]) == ress[2]["num_points"] and not ress[3]["stages"]["status"].any()
    assert (ress[3]["num_tracked"], ress[3]["num_points"], ress[3]["num_new"]) == (0, 0, 0) and ress[3]["reject"]["status"] == 2
    assert ress[4]["num_points"] >= 20 and not ress[4]["velocity_3d"].any() and ress[4]["ids"].min() == ress[0]["num_new"] + ress[1]["num_new"]
    assert not ress[5]["velocity_3d"].any()  # (in the map under -1)


def test_mixing_the_routes(eng, imgs):
    """Test 5: frames 0 - 2 through the call, frame 3 through the four separate calls on the table the call returned, then a reset and
    frames 3, 4 through the call again (the table can only be filled by the call itself: there is no "set table" entry)."""
    plain(eng)
    recs, _ = chain(eng, imgs[:4])
    ress = single(eng, imgs[:3])
    last = ress[2]
    cur, ids, cnt = last["pts"], last["ids"], last["track_cnt"]
    k = eng.klt_track(imgs[3], cur, want_iterations=False)
    ok = k["status"].astype(bool)
    assert same(k["next"], recs[3]["flow"]["next"]) and same(k["status"], recs[3]["flow"]["status"])
    cur, forw, ids, cnt = cur[ok], k["next"][ok], ids[ok], cnt[ok] + 1
    r = eng.track_reject(CAM, cur, forw, tf.draw(words(3), len(forw)))
    assert same(r["mask"], recs[3]["reject"]["out"]["mask"]) and r["num_inliers"] == recs[3]["reject"]["out"]["num_inliers"]
    ok = r["mask"].astype(bool)
    forw, ids, cnt = forw[ok], ids[ok], cnt[ok]
    g = eng.gft_detect(forw, cnt, **KW)
    assert same(g["kept"], recs[3]["detect"]["kept"]) and same(g["corners"], recs[3]["detect"]["corners"])
    forw = np.concatenate([forw[g["kept"]], g["corners"]]).astype(np.float32)
    ids = np.concatenate([ids[g["kept"]], np.full(len(g["corners"]), -1, np.int32)])
    u = eng.track_undistort(CAM, forw, ids, when(3))
    for key in ("un_pts", "un_pts_3d", "velocity_3d"):
        assert same(u[key], recs[3][key]), key
    assert recs[3]["velocity_3d"].any()
    # and back: a reset, then the call puts image 3 in place and tracks into image 4
    recs, _ = chain(eng, imgs[3:5], first=3)
    ress = single(eng, imgs[3:5], first=3)
    for j in range(2):
        agree(recs[j], ress[j], ("after the separate calls", j))


def sentinel():
    from lfvio import abi

    arrays = dict(pts=np.full((4096, 2), 7.5, np.float32), ids=np.full(4096, 77, np.int32), track_cnt=np.full(4096, 77, np.int32),
                  un_pts=np.full((4096, 2), 7.5, np.float32), un_pts_3d=np.full((4096, 3), 7.5, np.float32),
                  velocity_3d=np.full((4096, 3), 7.5, np.float32))
    out = abi.TrackFrameOutC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return arrays, out


def test_every_refused_field(eng, imgs):
    """Test 6."""
    from lfvio import abi

    plain(eng)
    want = single(eng, imgs[:3])
    single(eng, imgs[:2])
    count = want[1]["num_points"]
    assert count >= 20
    img, t, w = imgs[2], when(2), words(2)
    nan = float("nan")
    refused = [dict(width=15), dict(height=8193), dict(win_size=4), dict(win_size=43), dict(max_level=6), dict(max_level=-1), dict(max_iterations=0),
               dict(max_iterations=101), dict(epsilon=0.0), dict(epsilon=nan), dict(min_eig_threshold=-1.0), dict(max_count=0), dict(max_count=4097),
               dict(quality_level=0.0), dict(quality_level=1.5), dict(min_distance=-1), dict(min_distance=1025), dict(mask_radius=-1),
               dict(mask_radius=1025), dict(num_samples=0), dict(num_samples=1025), dict(capacity=MAX_CNT - 1), dict(capacity=4097),
               dict(max_count=10, capacity=count - 1)]
    n = 0
    for bad in refused:
        arrays, out = sentinel()
        head = bytes(out)[:abi.TrackFrameOutC.pts.offset]
        r = eng.track_frame(img, t, CAM, words=w, arrays=arrays, out=out, check=False, **dict(KW, **bad))
        assert r["rc"] == -1, bad
        assert bytes(out)[:len(head)] == head and all(np.all(a == (77 if a.dtype == np.int32 else 7.5)) for a in arrays.values()), bad
        n += 1
    others = [dict(img=None, params=dict(width=161, height=123)), dict(cam=None), dict(cam=dict(CAM, model=1)), dict(words=None, params=dict(num_samples=S)),
              dict(time=nan)] + [dict(null=(key,)) for key in TABLE]
    for bad in others:
        arrays, out = sentinel()
        head = bytes(out)[:abi.TrackFrameOutC.pts.offset]
        a = dict(img=img, time=t, cam=CAM, words=w, null=(), params={})
        a.update(bad)
        r = eng.track_frame(a["img"], a["time"], a["cam"], words=a["words"], arrays=arrays, out=out, null=a["null"], check=False, **dict(KW, **a["params"]))
        assert r["rc"] == -1, bad
        assert bytes(out)[:len(head)] == head and all(np.all(v == (77 if v.dtype == np.int32 else 7.5)) for v in arrays.values()), bad
        n += 1
    fin, out = abi.TrackFrameInC(), abi.TrackFrameOutC()
    assert eng.lib.lfvio_track_frame(eng.ctx, None, C.byref(out), None) == -1 and eng.lib.lfvio_track_frame(eng.ctx, C.byref(fin), None, None) == -1
    assert eng.lib.lfvio_track_frame(None, C.byref(fin), C.byref(out), None) == -1 and eng.lib.lfvio_track_frame_reset(None) == -1
    assert n >= 30
    # nothing resident moved: the table, n_id, the pyramid, the map and the time
    got = single(eng, imgs[2:3], first=2, reset=False)[0]
    for key in TABLE + ("num_points", "num_new", "num_tracked", "num_after_reject", "reject", "detect"):
        assert same(got[key], want[2][key]) if key in TABLE else repr(got[key]) == repr(want[2][key]), key
    assert got["velocity_3d"].any()
    # publish off needs no words
    assert eng.track_frame(imgs[3], when(3), CAM, publish=False, words=None, num_samples=S, **KW)["rc"] == 0


def flat(ress):
    return b"".join(np.ascontiguousarray(r[key]).tobytes() for r in ress for key in TABLE) + repr([(r["reject"]["status"], r["reject"]["best_sample"],
                                                                                                     r["detect"], r["num_new"]) for r in ress]).encode()


def test_repeatable_and_beside_an_optimization_in_flight(eng, imgs):
    """Test 7."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    plain(eng)
    alone = flat(single(eng, imgs[:3]))
    assert flat(single(eng, imgs[:3])) == alone
    w = synth.make_window(0, 300)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    sol0, prior0, _ = split(Engine(0), None)
    sol1, prior1, ress = split(Engine(0), lambda e: single(e, imgs[:3]))
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert flat(ress) == alone
