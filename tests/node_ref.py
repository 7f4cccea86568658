"""The node's loop around readImage (feature_tracker_node.cpp:28-62, :113-178) restated in numpy: what host/image_gate.h,
k_tf_message and host/feature_tracker.cpp are held to.

  Gate             img_callback's bookkeeping: the first image dropped, the discontinuity restart, the FREQ gate, the skipped first
                   publication
  rows_from_table  the nine-float rows of the feature message from one frame's table and undistortedPoints' outputs
  ImageNode        both around Engine.track_frame (the call WITHOUT the device's message), the sample words the raw outputs of
                   std::mt19937(seed): np.random.RandomState(seed).randint(0, 2**32, size=(S, 8), dtype=np.uint32)"""
import math

import numpy as np

DROP, RESTART, TRACKED, FIRST_PUBLICATION, PUBLISHED = 0, 1, 2, 3, 4


def c_round(x):
    """std::round: halves away from zero; inf and NaN pass."""
    if math.isnan(x) or math.isinf(x):
        return x
    return math.copysign(math.floor(abs(x) + 0.5), x)


class Gate:
    def __init__(self, freq=10):
        self.freq = freq
        self.first_image_flag, self.first_image_time, self.last_image_time, self.pub_count, self.init_pub = True, 0.0, 0.0, 1, False
        self.publish = False

    def state(self):
        return (self.first_image_flag, self.first_image_time, self.last_image_time, self.pub_count, self.init_pub, self.publish)

    def on_stamp(self, t):
        """-> DROP, RESTART or TRACKED (then self.publish is PUB_THIS_FRAME)."""
        t = float(t)
        if self.first_image_flag:
            self.first_image_flag, self.first_image_time, self.last_image_time = False, t, t
            return DROP
        if t - self.last_image_time > 1.0 or t < self.last_image_time:
            self.first_image_flag, self.last_image_time, self.pub_count = True, 0.0, 1
            return RESTART
        self.last_image_time = t
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.float64(1.0 * self.pub_count) / np.float64(t - self.first_image_time))  # IEEE: x / 0 = inf, 0 / 0 = NaN
        self.publish = bool(c_round(r) <= self.freq)
        if self.publish and abs(r - self.freq) < 0.01 * self.freq:
            self.first_image_time, self.pub_count = t, 0
        return TRACKED

    def after_frame(self):
        """Behind readImage: TRACKED, FIRST_PUBLICATION (the message is built and not sent) or PUBLISHED."""
        if not self.publish:
            return TRACKED
        self.pub_count += 1
        if not self.init_pub:
            self.init_pub = True
            return FIRST_PUBLICATION
        return PUBLISHED


def rows_from_table(pts, ids, cnt, un3d, vel):
    """[rows, 9] float32: un_pts_3d | (float)(id * NUM_OF_CAM + 0), NUM_OF_CAM = 1 | pts | velocity_3d of the entries with
    track_cnt > 1, in table order (feature_tracker_node.cpp:140-162)."""
    pts, un3d, vel = (np.asarray(a, np.float32).reshape(-1, k) for a, k in ((pts, 2), (un3d, 3), (vel, 3)))
    ids, cnt = np.asarray(ids, np.int32).reshape(-1), np.asarray(cnt, np.int32).reshape(-1)
    keep = cnt > 1
    rows = np.zeros((int(keep.sum()), 9), np.float32)
    rows[:, 0:3] = un3d[keep]
    rows[:, 3] = (ids[keep] * 1 + 0).astype(np.float32)  # int -> float32: nearest even
    rows[:, 4:6] = pts[keep]
    rows[:, 6:9] = vel[keep]
    return rows


class ImageNode:
    """img_callback over an Engine: on_image(t, img) -> (what, rows or None).  The engine's mask and CLAHE setting are set on the first
    image that reaches the tracker, as host/feature_tracker.cpp does."""

    def __init__(self, eng, cam, max_cnt=150, min_dist=30, freq=10, num_samples=100, seed=1, equalize=False, mask=None):
        self.eng, self.cam, self.gate = eng, cam, Gate(freq)
        self.kw = dict(max_count=max_cnt, min_distance=min_dist, mask_radius=min_dist)
        self.S, self.rng, self.equalize, self.mask, self.ready = num_samples, np.random.RandomState(seed), equalize, mask, False
        self.frames = []  # every frame's track_frame result
        eng.track_frame_reset()

    def on_image(self, t, img):
        what = self.gate.on_stamp(t)
        if what != TRACKED:
            return what, None
        if not self.ready:
            self.eng.gft_set_mask(self.mask)
            self.eng.clahe_set(3.0, (8, 8)) if self.equalize else self.eng.clahe_set(None)
            self.ready = True
        pub = self.gate.publish
        words = self.rng.randint(0, 2 ** 32, size=(self.S, 8), dtype=np.uint32) if pub else None
        r = self.eng.track_frame(img, float(t), self.cam, publish=pub, words=words, num_samples=self.S, **self.kw)
        self.frames.append(r)
        what = self.gate.after_frame()
        rows = rows_from_table(r["pts"], r["ids"], r["track_cnt"], r["un_pts_3d"], r["velocity_3d"]) if pub else None
        return what, (rows if what == PUBLISHED else None)
