"""The four camera models side by side, in the manner of time_camera.py: median / p95 over 200 calls after 20 warm-up calls of
(a) lfvio_track_reject at N = 200 matches, S = 100 sample sets and (b) lfvio_track_undistort of 200 points against a resident map of
200, for the PAL camera (OCam), EUROC (PINHOLE), MV3DM (MEI) and the three KANNALA_BRANDT calibrations of tests/kb_ref.py; (c)
lfvio_track_frame at 1280 x 960, MAX_CNT 150, MIN_DIST 30, S = 100 for one camera of each model with its centre moved to the image's:
200 frames after 20, three runs per camera, the cameras alternating.  The frames are time_track_frame.py's moving texture.  The calls
are synchronous, so wall time per call is the latency a tracker sees; the inputs of (a) and (b) alternate between two sets.  One JSON
line per measurement.

The file runs against a library from before the model existed too (an A/B run: copy it into that tree's tests/tools): a camera the
library refuses, or whose restatement the tree lacks, is reported as skipped."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import camera_ref as cr
import klt_ref as k
import track_ref as tr
from lfvio.engine import Engine
try:
    import kb_ref as kb
except ImportError:
    kb = None
eng = Engine(0)
N, S, CALLS, WARM, RUNS = int(os.environ.get("DBG_N", "200")), int(os.environ.get("DBG_S", "100")), 200, 20, int(os.environ.get("DBG_RUNS", "3"))
W, H = int(os.environ.get("DBG_W", "1280")), int(os.environ.get("DBG_H", "960"))
ids = np.arange(N, dtype=np.int32)
def stats(ts): return dict(median_us=round(float(np.median(ts)) * 1e6), p95_us=round(float(np.percentile(ts, 95)) * 1e6))
def loop(fn):
    ts, out = [], None
    for i in range(WARM + CALLS):
        t = time.perf_counter(); out = fn(i % 2, i); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, out
cams = dict(OCAM_PAL=(tr, tr.PAL), EUROC=(cr, cr.EUROC), MV3DM=(cr, cr.MV3DM))
if kb: cams.update(TUM=(kb, kb.TUM), CLA=(kb, kb.CLA), RSFISH=(kb, kb.RSFISH))
else: print(json.dumps(dict(camera="KANNALA_BRANDT", skipped="this tree has no tests/kb_ref.py")))
for name, (ref, cam) in cams.items():
    camc = eng.camera(cam)
    sets = [ref.make_matches(300 + j, cam, N) for j in range(2)]
    sm = [ref.make_samples(310 + j, N, S) for j in range(2)]
    rej, r = loop(lambda j, i: eng.track_reject(camc, sets[j][0], sets[j][1], sm[j]))
    eng.track_reset()
    und, u = loop(lambda j, i: eng.track_undistort(camc, sets[j][0], ids, 0.05 * i))
    print(json.dumps(dict(camera=name, N=N, S=S, reject=stats(rej), status=r["status"], inliers=r["num_inliers"], undistort=stats(und),
                          matched=int((u["matched"] >= 0).sum()))), flush=True)

MAX_CNT, MIN_DIST = 150, 30
f = k.texture(7)
imgs = [k.render(f, W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
walk = [0, 1, 2, 3, 2, 1]
words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
centre = dict(cx=W / 2.0, cy=H / 2.0)
frame_cams = dict(OCAM_PAL=dict(tr.PAL, **centre), EUROC=dict(cr.EUROC, **centre), MV3DM=dict(cr.MV3DM, **centre))
if kb: frame_cams.update(CLA=dict(kb.CLA, **centre), RSFISH=dict(kb.RSFISH, **centre))  # RSFISH: the corners lie beyond r_lim
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
                          frame_median_us=[x["median_us"] for x in v], frame_p95_us=[x["p95_us"] for x in v])), flush=True)
