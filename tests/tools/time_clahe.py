"""CLAHE at 1280 x 960, clip_limit 3.0, 8 x 8 tiles (the reference's call, feature_tracker.cpp:101-107), N = 200 points, win 41, 3
levels: median / p95 over 50 calls after 5 warm-up calls of (a) lfvio_klt_track with lfvio_clahe_set off, (b) the same with it on,
(c) lfvio_clahe_apply alone (image in, equalized image out, host buffers); the two images of a pure shift alternate as in time_klt.py.
Beside them the numpy restatement (tests/clahe_ref.py — numpy, not a tuned C++ build, and not OpenCV) on the same image.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_clahe.py` the kernels alone (DBG_REF_CALLS=0 leaves the restatement out,
DBG_SIZE=640x480 / DBG_N=... change the shape)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import clahe_ref as c
import klt_ref as k
from lfvio.engine import Engine
eng = Engine(0)
W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
N, WIN, LEVELS, CALLS, WARM = int(os.environ.get("DBG_N", "200")), 41, 3, 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "2"))
CLIP, TILES = 3.0, (8, 8)
f = k.texture(7)
fwd, inv = k.warp(W, H, (5.3, -3.6))
imgs = [k.render(f, W, H), k.render(f, W, H, inv)]
rng = np.random.default_rng(8)
m = (WIN - 1) // 2 + 4 + 7
p0 = np.stack([rng.uniform(m, W - 1 - m, N), rng.uniform(m, H - 1 - m, N)], axis=1).astype(np.float32)
pts = [p0, fwd(p0).astype(np.float32)]
def stats(ts): return f"median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us"
def track_loop():
    eng.klt_reset(); eng.klt_track(imgs[0], np.zeros((0, 2), np.float32), win_size=WIN, max_level=LEVELS)
    ts, out = [], None
    for i in range(WARM + CALLS):
        to = (i + 1) % 2
        t = time.perf_counter(); out = eng.klt_track(imgs[to], pts[1 - to], win_size=WIN, max_level=LEVELS); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, out
eng.clahe_set(None)
off, out_off = track_loop()
eng.clahe_set(CLIP, TILES)
on, out_on = track_loop()
level0 = eng.klt_level(0)  # of the last call: image (WARM + CALLS) % 2
eng.clahe_set(None)
ap, eq = [], None
for i in range(WARM + CALLS):
    t = time.perf_counter(); eq = eng.clahe_apply(imgs[0], CLIP, TILES); dt = time.perf_counter() - t
    if i >= WARM: ap.append(dt)
line = (f"{W}x{H} clip={CLIP} tiles={TILES[0]}x{TILES[1]} N={N} win={WIN}: lfvio_klt_track, setting off {stats(off)} (tracked {out_off['num_tracked']}); "
        f"setting on {stats(on)} (tracked {out_on['num_tracked']}); lfvio_clahe_apply alone {stats(ap)} per call (host buffers)")
rs = []
for _ in range(REF_CALLS):
    t = time.perf_counter(); ref = c.clahe(imgs[0], CLIP, TILES)[0]; rs.append(time.perf_counter() - t)
if rs:
    same = np.array_equal(eq, ref) and np.array_equal(level0, c.clahe(imgs[(WARM + CALLS) % 2], CLIP, TILES)[0])
    line += f"; numpy restatement median {np.median(rs)*1e3:.0f} ms, same bits: {same}"
print(line)
