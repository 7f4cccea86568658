"""One image through FeatureTracker::readImage as device calls only — the PYTHON chain the tests hold the stages against.

What readImage (feature_tracker/src/feature_tracker.cpp:95-184) and the node's updateID loop (feature_tracker_node.cpp:102-111) do, in
their order, on an Engine: the CLAHE setting is the engine's own (Engine.clahe_set), then

  1. klt_track and reduceVector by its status (the inBorder test is the call's);
  2. track_cnt++;
  3. when publishing: track_reject and reduceVector by its mask (the sample sets are drawn here from a seeded generator, 8 distinct
     indices each; with fewer than 8 matches the call rejects nothing), then gft_detect — setMask reorders the survivors by falling
     track_cnt — and the new corners with id -1 and count 1;
  4. cur_pts = forw_pts, track_undistort;
  5. the numbering: every id that is -1 takes the next number.

The product's tracker is the host class around the same calls; this module exists so that the chain can be tested stage by stage
(tests/test_tracker_chain.py): every frame leaves a record of each stage's inputs and outputs."""
import numpy as np


class FeatureTracker:
    def __init__(self, eng, cam, max_cnt=150, min_dist=30, num_samples=100, seed=0, klt=None):
        """cam: the camera of Engine.camera(); klt: keyword arguments of Engine.klt_track (win_size, max_level, ...)."""
        self.eng, self.cam, self.max_cnt, self.min_dist, self.num_samples = eng, cam, max_cnt, min_dist, num_samples
        self.rng = np.random.default_rng(seed)
        self.klt = dict(klt or {})
        self.cur_pts = np.zeros((0, 2), np.float32)
        self.ids, self.track_cnt = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.n_id = 0
        self.records = []
        eng.klt_reset()
        eng.track_reset()

    def draw_samples(self, n):
        return np.stack([self.rng.choice(n, 8, replace=False) for _ in range(self.num_samples)]).astype(np.int32)

    def read_image(self, img, time, publish=True):
        """Returns the frame's record: flow, reject and detect (None when not publishing), undistort, and the state after the
        numbering (cur_pts, ids, track_cnt, un_pts, un_pts_3d, velocity_3d)."""
        eng, rec = self.eng, dict(time=float(time), publish=bool(publish), reject=None, detect=None)
        cur, ids, cnt = self.cur_pts, self.ids, self.track_cnt
        k = eng.klt_track(img, cur, want_iterations=False, **self.klt)
        ok = k["status"].astype(bool)
        rec["flow"] = dict(prev_pts=cur.copy(), next=k["next"].copy(), status=k["status"].copy())
        cur, forw, ids, cnt = cur[ok], k["next"][ok], ids[ok], cnt[ok]
        cnt = cnt + 1
        if publish:
            samples = self.draw_samples(len(forw)) if len(forw) >= 8 else None
            r = eng.track_reject(self.cam, cur, forw, samples)
            rec["reject"] = dict(cur=cur.copy(), forw=forw.copy(), samples=samples, out=r)
            ok = r["mask"].astype(bool)
            cur, forw, ids, cnt = cur[ok], forw[ok], ids[ok], cnt[ok]
            g = eng.gft_detect(forw, cnt, max_count=self.max_cnt, min_distance=self.min_dist, mask_radius=self.min_dist)
            rec["detect"] = dict(pts=forw.copy(), track_cnt=cnt.copy(), kept=g["kept"].copy(), corners=g["corners"].copy())
            kept, new = g["kept"], len(g["corners"])
            forw = np.concatenate([forw[kept], g["corners"]]).astype(np.float32)
            ids = np.concatenate([ids[kept], np.full(new, -1, np.int32)])
            cnt = np.concatenate([cnt[kept], np.ones(new, np.int32)])
        u = eng.track_undistort(self.cam, forw, ids, time)
        rec["undistort"] = dict(pts=forw.copy(), ids=ids.copy(), time=float(time), out=u)
        ids = ids.copy()
        for i in np.flatnonzero(ids == -1):
            ids[i], self.n_id = self.n_id, self.n_id + 1
        self.cur_pts, self.ids, self.track_cnt = forw, ids, cnt
        rec.update(cur_pts=forw.copy(), ids=ids.copy(), track_cnt=cnt.copy(), un_pts=u["un_pts"], un_pts_3d=u["un_pts_3d"],
                   velocity_3d=u["velocity_3d"])
        self.records.append(rec)
        return rec
