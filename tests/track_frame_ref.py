"""numpy restatement of lfvio_track_frame (include/lfvio.h): one image through FeatureTracker::readImage
(feature_tracker/src/feature_tracker.cpp:95-184) and updateID (feature_tracker_node.cpp:102-111) on a resident track table.  The
frame COMPOSES the restatements of its stages — klt_ref (the flow), track_ref (rejectWithF, undistortedPoints), gft_ref (setMask,
goodFeaturesToTrack), clahe_ref where an equalizer is set — and adds what is new in the specification:

  draw(words, n)        the sample sets from [S, 8] uint32 words over n >= 8 matches: for k = 0 .. 7, r = words[s][k] % (n - k); for
                        every index c already chosen for the set, in ascending order, if r >= c: r += 1; samples[s][k] = r
  Frame                 the state object: the table (cur_pts, ids, track_cnt), n_id, the previous image's pyramid and the
                        undistortedPoints map; Frame.read(img, time, cam, publish, words, **params) is one call
  check(...)            the argument check of trackframe_plan.h, field by field; True: refused

A camera is track_ref's dict."""
import numpy as np

import gft_ref
import klt_ref
import track_ref as tr

MAX_POINTS, MAX_SAMPLES, MIN_MATCHES = tr.MAX_POINTS, tr.MAX_SAMPLES, tr.MIN_MATCHES
DEFAULTS = dict(win_size=41, max_level=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, border=1, max_count=150, quality_level=0.01,
                min_distance=30, mask_radius=30)


def draw(words, n):
    """[S, 8] int32 sample sets over n >= 8 matches from [S, 8] uint32 words."""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 8)
    out = np.zeros(words.shape, np.int32)
    for s, row in enumerate(words):
        chosen = []
        for k in range(8):
            r = int(row[k]) % (n - k)
            for c in sorted(chosen):
                if r >= c:
                    r += 1
            chosen.append(r)
            out[s, k] = r
    return out


def check(p, table_count, have_image=True, cam=tr.PAL, have_words=True, publish=True, time=0.0):
    """p: dict with width, height, the keys of DEFAULTS, num_samples and capacity.  In the order of trackframe_plan.h: the fields
    of lfvio_klt_track, of lfvio_gft_detect, the camera, then the frame's own."""
    if not (16 <= p["width"] <= 8192 and 16 <= p["height"] <= 8192) or not have_image:
        return True
    if p["win_size"] < 5 or p["win_size"] > 41 or p["win_size"] % 2 == 0 or not 0 <= p["max_level"] <= klt_ref.MAX_LEVEL:
        return True
    if not 1 <= p["max_iterations"] <= 100 or not p["epsilon"] > 0.0 or not p["min_eig_threshold"] >= 0.0:
        return True
    if not 1 <= p["max_count"] <= MAX_POINTS or not 0.0 < p["quality_level"] <= 1.0:
        return True
    if not 0 <= p["min_distance"] <= 1024 or not 0 <= p["mask_radius"] <= 1024:
        return True
    if tr.common_check(cam, 0):
        return True
    if not 1 <= p["num_samples"] <= MAX_SAMPLES or (publish and not have_words):
        return True
    if p["capacity"] < max(p["max_count"], table_count) or p["capacity"] > MAX_POINTS:
        return True
    return bool(np.isnan(time))


class Frame:
    def __init__(self, base_mask=None, equalize=None):
        """base_mask: lfvio_gft_set_mask's; equalize: a function image -> image (clahe_ref's, with lfvio_clahe_set's setting)."""
        self.base, self.equalize = base_mask, equalize
        self.reset()

    def reset(self):
        self.pts, self.ids, self.cnt = np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.n_id, self.prev, self.undistort = 0, None, tr.Undistort()

    def read(self, img, time, cam, publish=True, words=None, **params):
        p = dict(DEFAULTS, **params)
        img = np.asarray(img, np.uint8) if self.equalize is None else self.equalize(np.asarray(img, np.uint8))
        pyr = klt_ref.pyramid(img, p["win_size"], p["max_level"])
        prev = pyr if self.prev is None or self.prev[0].shape != pyr[0].shape else self.prev
        cur, ids, cnt = self.pts, self.ids, self.cnt
        # 1, 2
        k = klt_ref.track(prev, pyr, cur, win=p["win_size"], max_level=p["max_level"], max_iterations=p["max_iterations"], epsilon=p["epsilon"],
                          min_eig_threshold=p["min_eig_threshold"], border=p["border"])
        ok = k["status"].astype(bool)
        cur, forw, ids, cnt = cur[ok], k["next"][ok], ids[ok], cnt[ok] + 1
        rec = dict(next=k["next"], status=k["status"], num_tracked=len(forw), samples=None, reject=None, detect=None)
        if publish:
            # 3
            if len(forw) >= MIN_MATCHES:
                rec["samples"] = draw(words, len(forw))
            r = tr.reject(cam, cur, forw, rec["samples"])
            rec["reject"] = r
            ok = r["mask"].astype(bool)
            forw, ids, cnt = forw[ok], ids[ok], cnt[ok]
            # 4
            g = gft_ref.gft(img, base=self.base, pts=forw, cnt=cnt, max_count=p["max_count"], quality=p["quality_level"],
                            min_distance=p["min_distance"], mask_radius=p["mask_radius"])
            rec["detect"] = g
            kept, corners = np.asarray(g["kept"], np.int64), np.asarray(g["corners"], np.float32).reshape(-1, 2)
            forw = np.concatenate([forw[kept], corners]).astype(np.float32)
            ids = np.concatenate([ids[kept], np.full(len(corners), -1, np.int32)])
            cnt = np.concatenate([cnt[kept], np.ones(len(corners), np.int32)])
        rec["num_after_reject"] = len(forw) if not publish else int(rec["reject"]["mask"].sum())
        # 5: the ids as they are now, the -1 included
        u = self.undistort(cam, forw, ids, time)
        # 6
        ids = ids.copy()
        new = np.flatnonzero(ids == -1)
        ids[new] = self.n_id + np.arange(len(new), dtype=np.int32)
        self.n_id += len(new)
        self.pts, self.ids, self.cnt, self.prev = forw, ids, cnt.astype(np.int32), pyr
        rec.update(pts=forw, ids=ids, track_cnt=self.cnt, num_new=len(new), un_pts=u["un_pts"], un_pts_3d=u["un_pts_3d"], velocity_3d=u["velocity_3d"])
        return rec
