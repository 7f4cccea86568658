"""rejectWithF and undistortedPoints at N = 200 matches, S = 100 sample sets (the reference's), the PAL camera: median / p95 over 200
calls after 20 warm-up calls of (a) lfvio_track_reject (pixels in, mask out), (b) today's route before it: the lift on the host (the
numpy restatement, tests/track_ref.py — numpy, not a tuned C++ build) and lfvio_two_view on the lifted bearings, the two timed
separately, (c) lfvio_track_undistort of 200 points against a resident map of 200.  The calls are synchronous (each ends with its copy
down and a stream synchronisation), so wall time per call is the latency a tracker sees; the inputs alternate between two sets so that
no call repeats the one before.  Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_track.py` the kernels alone
(DBG_N=... / DBG_S=... change the shape)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import track_ref as tr
from lfvio.engine import Engine
eng = Engine(0)
N, S, CALLS, WARM = int(os.environ.get("DBG_N", "200")), int(os.environ.get("DBG_S", "100")), 200, 20
cam = tr.PAL
camc = eng.camera(cam)
sets = [tr.make_matches(300 + k, cam, N) + (tr.make_samples(310 + k, N, S),) for k in range(2)]
lifted = [(tr.bearings(cam, c), tr.bearings(cam, f)) for c, f, _ in sets]
ids = np.arange(N, dtype=np.int32)
def stats(ts): return f"median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us"
def loop(fn):
    ts, out = [], None
    for i in range(WARM + CALLS):
        t = time.perf_counter(); out = fn(i % 2, i); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, out
rej, r = loop(lambda k, i: eng.track_reject(camc, sets[k][0], sets[k][1], sets[k][2]))
tvw, t2 = loop(lambda k, i: eng.two_view(lifted[k][0], lifted[k][1], sets[k][2]))
lift, _ = loop(lambda k, i: (tr.bearings(cam, sets[k][0]), tr.bearings(cam, sets[k][1])))
eng.track_reset()
und, u = loop(lambda k, i: eng.track_undistort(camc, sets[k][0], ids, 0.05 * i))
same = r["status"] == t2["status"] and np.array_equal(r["mask"], t2["mask"]) and r["best_sample"] == t2["best_sample"]
print(f"N={N} S={S}: lfvio_track_reject {stats(rej)} (status {r['status']}, {r['num_inliers']} inliers); lfvio_two_view on the same matches "
      f"{stats(tvw)} + host lift (numpy) {stats(lift)}, same mask: {same}; lfvio_track_undistort {N} against {N} {stats(und)} "
      f"({int((u['matched'] >= 0).sum())} matched)")
