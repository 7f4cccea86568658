"""lfvio_klt_track at 1280 x 960, N = 200 points, win 41, 3 levels (the reference's call, feature_tracker.cpp:127): median / p95 of the
whole call (image and points in, points / status / iterations out, host buffers) over 50 calls after 5 warm-up calls, the two images
of a pure shift alternating so that every call tracks a real flow from the resident pyramid; beside it the numpy restatement
(tests/klt_ref.py — numpy, not a tuned C++ build, and not OpenCV) on the same pair, pyramids included.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_klt.py` the kernels alone (DBG_REF_CALLS=0 leaves the restatement out,
DBG_SIZE=640x480 / DBG_N=... change the shape)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import klt_ref as k
from lfvio.engine import Engine
eng = Engine(0)
W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
N, WIN, LEVELS, CALLS, WARM = int(os.environ.get("DBG_N", "200")), 41, 3, 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "2"))
SHIFT = (5.3, -3.6)
f = k.texture(7)
fwd, inv = k.warp(W, H, SHIFT)
imgs = [k.render(f, W, H), k.render(f, W, H, inv)]
rng = np.random.default_rng(8)
m = (WIN - 1) // 2 + 4 + 7
p0 = np.stack([rng.uniform(m, W - 1 - m, N), rng.uniform(m, H - 1 - m, N)], axis=1).astype(np.float32)
pts = [p0, fwd(p0).astype(np.float32)]  # the points of image 0, and where they are in image 1 (tracked back by the calls into image 0)
eng.klt_track(imgs[0], np.zeros((0, 2), np.float32), win_size=WIN, max_level=LEVELS)
ts, out = [], [None, None]
for i in range(WARM + CALLS):
    to = (i + 1) % 2
    t = time.perf_counter(); out[to] = eng.klt_track(imgs[to], pts[1 - to], win_size=WIN, max_level=LEVELS); dt = time.perf_counter() - t
    if i >= WARM: ts.append(dt)
err = np.hypot(*(out[1]["next"] - fwd(p0)).T).max()
line = (f"{W}x{H} N={N} win={WIN} levels={out[1]['levels_used']}: lfvio_klt_track median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us "
        f"per call (host buffers); tracked {out[1]['num_tracked']}, iterations per point (all levels) mean {out[1]['iterations'].sum(axis=1).mean():.1f}, "
        f"worst distance to the true flow {err:.3f} px")
rs = []
for _ in range(REF_CALLS):
    t = time.perf_counter(); ref = k.track(k.pyramid(imgs[0], WIN, LEVELS), k.pyramid(imgs[1], WIN, LEVELS), p0, win=WIN, max_level=LEVELS); rs.append(time.perf_counter() - t)
if rs:
    d = np.hypot(*(out[1]["next"].astype(np.float64) - ref["next"]).T).max()
    line += (f"; numpy restatement median {np.median(rs)*1e3:.0f} ms, same status: {np.array_equal(out[1]['status'], ref['status'])}, "
             f"same iteration counts: {np.array_equal(out[1]['iterations'], ref['iterations'])}, worst distance {d:.2e} px")
print(line)
