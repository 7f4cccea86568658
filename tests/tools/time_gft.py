"""lfvio_gft_detect at 1280 x 960 with 150 tracked points, max_count 150, min_distance = mask_radius = 30 (the reference's call,
feature_tracker.cpp:46-83, :147-176): median / p95 of the whole call (points and counts in, kept indices and corners out, host
buffers; the image is resident) over 50 calls after 5 warm-up calls; beside it the numpy restatement (tests/gft_ref.py — numpy, not a
tuned C++ build, and not OpenCV) on the same input, response included.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_gft.py` the kernels alone (DBG_REF_CALLS=0 leaves the restatement out,
DBG_SIZE=640x480 / DBG_N=... change the shape)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gft_ref as g
from lfvio.engine import Engine
eng = Engine(0)
W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
N, MC, D, CALLS, WARM = int(os.environ.get("DBG_N", "150")), 150, 30, 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "2"))
img = g.textured(W, H, 7)
pts, cnt = g.tracked_case(W, H, 8, n=N)
eng.klt_track(img, np.zeros((0, 2), np.float32))
ts, out = [], None
for i in range(WARM + CALLS):
    t = time.perf_counter(); out = eng.gft_detect(pts, cnt, max_count=MC, min_distance=D, mask_radius=D); dt = time.perf_counter() - t
    if i >= WARM: ts.append(dt)
line = (f"{W}x{H} N={N} max_count={MC} d={D}: lfvio_gft_detect median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call "
        f"(host buffers, image resident); kept {len(out['kept'])}, corners {len(out['corners'])} of {out['num_candidates']} candidates")
rs = []
for _ in range(REF_CALLS):
    t = time.perf_counter(); ref = g.gft(img, None, pts, cnt, max_count=MC, min_distance=D, mask_radius=D); rs.append(time.perf_counter() - t)
if rs:
    same = (np.array_equal(out["kept"], ref["kept"]) and out["corners"].tobytes() == ref["corners"].tobytes() and out["num_candidates"] == ref["num_candidates"]
            and out["max_response"] == ref["max_response"])
    line += f"; numpy restatement median {np.median(rs)*1e3:.0f} ms, same bits: {same}"
print(line)
