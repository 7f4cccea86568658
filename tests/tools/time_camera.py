"""The three camera models side by side, in the manner of time_track.py: median / p95 over 200 calls after 20 warm-up calls of
(a) lfvio_track_reject at N = 200 matches, S = 100 sample sets and (b) lfvio_track_undistort of 200 points against a resident map of
200, for the PAL camera (OCam) and the five cameras of tests/camera_ref.py (PINHOLE and MEI, with and without distortion, xi = 1);
(c) lfvio_track_frame at 752 x 480, MAX_CNT 150, MIN_DIST 30, S = 100 for EUROC and MV3DM and, on the same frames, the PAL camera with
its centre moved to the image's: 200 frames after 20, three runs per camera, the cameras alternating.  The frames are
time_track_frame.py's moving texture.  The calls are synchronous, so wall time per call is the latency a tracker sees; the inputs of
(a) and (b) alternate between two sets.  One JSON line per measurement."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import camera_ref as cr
import klt_ref as k
import track_ref as tr
from lfvio.engine import Engine
eng = Engine(0)
N, S, CALLS, WARM, RUNS = int(os.environ.get("DBG_N", "200")), int(os.environ.get("DBG_S", "100")), 200, 20, int(os.environ.get("DBG_RUNS", "3"))
ids = np.arange(N, dtype=np.int32)
def stats(ts): return dict(median_us=round(float(np.median(ts)) * 1e6), p95_us=round(float(np.percentile(ts, 95)) * 1e6))
def loop(fn):
    ts, out = [], None
    for i in range(WARM + CALLS):
        t = time.perf_counter(); out = fn(i % 2, i); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, out
cams = dict(OCAM_PAL=tr.PAL, **cr.CAMERAS)
for name, cam in cams.items():
    camc = eng.camera(cam)
    sets = [cr.make_matches(300 + j, cam, N) if name != "OCAM_PAL" else tr.make_matches(300 + j, cam, N) for j in range(2)]
    sm = [cr.make_samples(310 + j, N, S) for j in range(2)]
    rej, r = loop(lambda j, i: eng.track_reject(camc, sets[j][0], sets[j][1], sm[j]))
    eng.track_reset()
    und, u = loop(lambda j, i: eng.track_undistort(camc, sets[j][0], ids, 0.05 * i))
    print(json.dumps(dict(camera=name, N=N, S=S, reject=stats(rej), status=r["status"], inliers=r["num_inliers"], undistort=stats(und),
                          matched=int((u["matched"] >= 0).sum()))))

W, H, MAX_CNT, MIN_DIST = 752, 480, 150, 30
f = k.texture(7)
imgs = [k.render(f, W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
walk = [0, 1, 2, 3, 2, 1]
words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
frame_cams = dict(EUROC=cr.EUROC, MV3DM=cr.MV3DM, OCAM_PAL=dict(tr.PAL, cx=W / 2.0, cy=H / 2.0))
res, pts = {}, {}
for _ in range(RUNS):
    for name, cam in frame_cams.items():
        camc = eng.camera(cam)
        eng.track_frame_reset()
        ts = []
        for i in range(WARM + CALLS):
            t = time.perf_counter(); r = eng.track_frame(imgs[walk[i % 6]], 0.05 * i, camc, words=words[i % 8], **KW); dt = time.perf_counter() - t
            if i >= WARM: ts.append(dt)
        res.setdefault(name, []).append(stats(ts))
        pts[name] = (r["num_points"], r["reject"]["status"])
for name, v in res.items():
    print(json.dumps(dict(camera=name, size=f"{W}x{H}", max_cnt=MAX_CNT, samples=S, points=pts[name][0], reject_status=pts[name][1],
                          frame_median_us=[x["median_us"] for x in v], frame_p95_us=[x["p95_us"] for x in v])))
