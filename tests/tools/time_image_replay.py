"""Measurements of the image route, one JSON line each.

  call       lfvio_track_frame_message beside lfvio_track_frame at 1280 x 960, MAX_CNT 150, MIN_DIST 30, S = 100, the PAL camera: median /
             p95 per frame over 200 frames after 20 warm-up frames, three runs of each, alternating in one process on the frames of
             tests/tools/time_track_frame.py.  DBG_PARENT_LIB = a build of the parent commit's library: its lfvio_track_frame is a
             third route.  Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_image_replay.py` with DBG_PART=call and
             DBG_ROUTE=message the kernels of that route alone (k_tf_message among them).
  recording  a make_image_stream recording through HostEstimator.replay_images: tracker milliseconds per raw image (track_stats) and
             wall-clock milliseconds per raw image end to end, at DBG_SCALES (default 4,1: 320 x 240 with the GPU test's settings,
             1280 x 960 with MAX_CNT 150, MIN_DIST 30), the second of two runs (the first one pays the allocations)."""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
PARTS = os.environ.get("DBG_PART", "call,recording").split(",")

if "call" in PARTS:
    import klt_ref as k
    import track_ref as tr
    from lfvio.engine import Engine
    W, H, MAX_CNT, MIN_DIST, S, FRAMES, WARM, RUNS = 1280, 960, 150, 30, 100, 200, 20, int(os.environ.get("DBG_RUNS", "3"))
    ROUTES = os.environ.get("DBG_ROUTE", "frame,message").split(",")
    engines = {r: Engine(0) for r in ROUTES}
    if os.environ.get("DBG_PARENT_LIB"):
        engines["parent"] = Engine(0, lib_path=os.environ["DBG_PARENT_LIB"])
    f = k.texture(7)
    imgs = [k.render(f, W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
    walk = [0, 1, 2, 3, 2, 1]
    words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
    KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)

    def run(route):
        eng = engines[route]
        cam = eng.camera(tr.PAL)
        call = eng.track_frame
        if route == "message":  # (the rows' array allocated once, as a caller would: a fresh 147 KB array a frame costs more than the kernel)
            buf = np.zeros((4096, 9), np.float32)
            call = lambda *a, **kw: eng.track_frame_message(*a, rows=buf, **kw)
        eng.track_frame_reset()
        ts, r = [], None
        for i in range(WARM + FRAMES):
            img, w = imgs[walk[i % 6]], words[i % 8]
            t = time.perf_counter(); r = call(img, 0.05 * i, cam, words=w, **KW); dt = time.perf_counter() - t
            if i >= WARM: ts.append(dt)
        return ts, r

    res, last = {}, {}
    for _ in range(RUNS):  # (the routes alternate)
        for route in engines:
            ts, last[route] = run(route)
            res.setdefault(route, []).append((float(np.median(ts)) * 1e6, float(np.percentile(ts, 95)) * 1e6))
    line = dict(part="call", size=f"{W}x{H}", max_cnt=MAX_CNT, samples=S, points=int(next(iter(last.values()))["num_points"]))
    for route, v in res.items():
        line[route + "_median_us"], line[route + "_p95_us"] = [round(m) for m, _ in v], [round(p) for _, p in v]
    if "message" in last:
        line["rows"] = int(last["message"]["num_rows"])
    tabs = [b"".join(np.ascontiguousarray(r[key]).tobytes() for key in ("pts", "ids", "track_cnt", "un_pts_3d", "velocity_3d")) for r in last.values()]
    line["same_tables"] = all(t == tabs[0] for t in tabs)
    print(json.dumps(line), flush=True)
    for e in engines.values():
        e.close()

if "recording" in PARTS:
    from lfvio import trace
    from lfvio.engine import Engine  # noqa: F401  (torch first: the ROCm wheel brings its own HIP runtime)
    from lfvio.host import HostEstimator
    import ate
    d = tempfile.mkdtemp(prefix="image_replay_")
    for scale in [int(s) for s in os.environ.get("DBG_SCALES", "4,1").split(",")]:
        n = int(os.environ.get("DBG_FRAMES", "36" if scale > 1 else "16"))
        src, traj = os.path.join(d, f"s{scale}.lfvt"), os.path.join(d, f"s{scale}.txt")
        made = trace.make_image_stream(src, seed=0, n_frames=n, scale=scale)
        kw = dict(max_cnt=80, min_dist=12) if scale > 1 else dict(max_cnt=150, min_dist=30)
        he = HostEstimator()
        he.clear_state(); he.set_min_parallax(10.0); he.set_solver_time(0.0)
        he.track_config(made["camera"], freq=10, num_samples=100, seed=77, annulus=made["annulus"], **kw)
        he.replay_images(src, "")  # (the first recording pays for the context's buffers)
        he.clear_state()
        t = time.perf_counter(); rc, st, ts = he.replay_images(src, traj); wall = (time.perf_counter() - t) * 1e3
        he.close()
        err = ate.ate(traj, src) if st["poses"] >= 3 else None
        print(json.dumps(dict(part="recording", size=f"{made['width']}x{made['height']}", raw_images=int(ts["raw_images"]), published=int(ts["published"]),
                              rows_per_message=round(ts["rows"] / max(ts["published"], 1), 1), rc=rc, poses=st["poses"], bootstraps=st["bootstraps"],
                              failures=st["failures"], tracker_ms_per_raw_image=round(ts["tracker_ms"] / ts["raw_images"], 3),
                              end_to_end_ms_per_raw_image=round(wall / ts["raw_images"], 3), ate_rmse_m=None if err is None else round(err["rmse"], 4),
                              ate_n=None if err is None else err["n"], **kw)), flush=True)
