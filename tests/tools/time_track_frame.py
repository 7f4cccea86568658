"""lfvio_track_frame against the four-call chain at 1280 x 960, MAX_CNT 150, MIN_DIST 30, S = 100, the PAL camera, CLAHE off and on:
median / p95 per frame over 200 frames after 20 warm-up frames, three runs of each route on the same frames in the same process.
The frames are four klt_ref-rendered images of a slowly moving texture walked back and forth, so that every frame tracks a real
flow and detects a few new corners.  (a) the single call: wall time of Engine.track_frame.  (b) the chain, the parent's route:
lfvio_klt_track, lfvio_track_reject, lfvio_gft_detect and lfvio_track_undistort through Engine, the SUM of the four calls' wall times;
what the host does between them (reduceVector, drawing the sample sets, the numbering — numpy and Python here) is not counted.  Both
routes get the same words, and the last frame's tables are compared.  Under `rocprofv3 --kernel-trace --stats -- python
tests/tools/time_track_frame.py` with DBG_ROUTE=frame (or chain) and DBG_CLAHE=0 / 1 the kernels of one route alone."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import klt_ref as k
import track_frame_ref as tf
import track_ref as tr
from lfvio.engine import Engine
eng = Engine(0)
W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
MAX_CNT, MIN_DIST, S, FRAMES, WARM, RUNS = int(os.environ.get("DBG_N", "150")), 30, 100, 200, 20, int(os.environ.get("DBG_RUNS", "3"))
ROUTES = os.environ.get("DBG_ROUTE", "frame,chain").split(",")
CLAHE = [bool(int(x)) for x in os.environ.get("DBG_CLAHE", "0,1").split(",")]
cam = eng.camera(tr.PAL)
f = k.texture(7)
imgs = [k.render(f, W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
walk = [0, 1, 2, 3, 2, 1]
words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)

def run_frame():
    eng.track_frame_reset()
    ts, r = [], None
    for i in range(WARM + FRAMES):
        img, w = imgs[walk[i % 6]], words[i % 8]
        t = time.perf_counter(); r = eng.track_frame(img, 0.05 * i, cam, words=w, **KW); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, (r["pts"].copy(), r["ids"].copy(), r["track_cnt"].copy(), r["velocity_3d"].copy())

def run_chain():
    eng.klt_reset(); eng.track_reset()
    cur, ids, cnt, n_id, ts = np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, []
    for i in range(WARM + FRAMES):
        img, w = imgs[walk[i % 6]], words[i % 8]
        t0 = time.perf_counter(); kk = eng.klt_track(img, cur, want_iterations=False); dt = time.perf_counter() - t0
        ok = kk["status"].astype(bool)
        cur, forw, ids, cnt = cur[ok], kk["next"][ok], ids[ok], cnt[ok] + 1
        sm = tf.draw(w, len(forw)) if len(forw) >= 8 else None
        t0 = time.perf_counter(); r = eng.track_reject(cam, cur, forw, sm); dt += time.perf_counter() - t0
        ok = r["mask"].astype(bool)
        forw, ids, cnt = forw[ok], ids[ok], cnt[ok]
        t0 = time.perf_counter(); g = eng.gft_detect(forw, cnt, **KW); dt += time.perf_counter() - t0
        new = len(g["corners"])
        forw = np.concatenate([forw[g["kept"]], g["corners"]]).astype(np.float32)
        ids = np.concatenate([ids[g["kept"]], np.full(new, -1, np.int32)])
        cnt = np.concatenate([cnt[g["kept"]], np.ones(new, np.int32)])
        t0 = time.perf_counter(); u = eng.track_undistort(cam, forw, ids, 0.05 * i, want_matched=False); dt += time.perf_counter() - t0
        fresh = np.flatnonzero(ids == -1)
        ids[fresh] = n_id + np.arange(len(fresh), dtype=np.int32); n_id += len(fresh)
        cur = forw
        if i >= WARM: ts.append(dt)
    return ts, (cur.copy(), ids.copy(), cnt.astype(np.int32), u["velocity_3d"].copy())

for clahe in CLAHE:
    eng.clahe_set(3.0, (8, 8)) if clahe else eng.clahe_set(None)
    res, last = {}, {}
    for _ in range(RUNS):  # (the routes alternate)
        for route in ROUTES:
            ts, last[route] = (run_frame if route == "frame" else run_chain)()
            res.setdefault(route, []).append((float(np.median(ts)) * 1e6, float(np.percentile(ts, 95)) * 1e6))
    line = dict(size=f"{W}x{H}", max_cnt=MAX_CNT, samples=S, clahe=clahe, points=int(len(next(iter(last.values()))[1])))
    for route, v in res.items():
        line[route + "_median_us"], line[route + "_p95_us"] = [round(m) for m, _ in v], [round(p) for _, p in v]
    if len(last) == 2:
        line["same_tables"] = all(a.tobytes() == b.tobytes() for a, b in zip(last["frame"], last["chain"]))
        med = {r: np.median([m for m, _ in v]) for r, v in res.items()}
        line["chain_minus_frame_us"] = round(float(med["chain"] - med["frame"]))
        line["chain_spread_us"] = round(max(m for m, _ in res["chain"]) - min(m for m, _ in res["chain"]))
    print(json.dumps(line))
