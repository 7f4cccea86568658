"""lfvio_track_batch_frame against the parent's route for several streams — B contexts in the same process, each given its frame
through lfvio_track_frame_message in turn — at 1280 x 960, MAX_CNT 150, MIN_DIST 30, S = 100, the PAL camera, a distinct texture per
slot, for B = 1, 4, 16, 64.  Wall time per batch call (for the turn-taking route: per round of B calls), median and p95 over 200
calls after 20 warm-up calls, three runs of each route, alternating.  Both routes are timed at the C entry with every struct built
beforehand, so neither pays for Python's packing; both get the same images, times and words, and the last call's tables are compared.
Every slot's two images (klt_ref-rendered, a slowly moving texture, walked back and forth so that every frame tracks a real flow) are
rendered by a pool of processes BEFORE the device is opened.  One JSON line per B with both routes' frames per second and
`batch_below_turns`: every run of the batch below every run of the turn-taking route.  DBG_B=16 (a list) picks the sizes, DBG_ROUTE=batch
or turns one route alone, as for a `rocprofv3 --kernel-trace --stats -- python tests/tools/time_track_batch.py` run."""
import ctypes as C, json, os, sys, time
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import klt_ref as k
import track_ref as tr

W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
MAX_CNT, MIN_DIST, S, CALLS, WARM, RUNS = int(os.environ.get("DBG_N", "150")), 30, 100, int(os.environ.get("DBG_CALLS", "200")), 20, int(os.environ.get("DBG_RUNS", "3"))
SIZES = [int(x) for x in os.environ.get("DBG_B", "1,4,16,64").split(",")]
ROUTES = os.environ.get("DBG_ROUTE", "batch,turns").split(",")


def render(job):
    slot, j = job
    return k.render(k.texture(100 + slot), W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1])


def main():
    jobs = [(slot, j) for slot in range(max(SIZES)) for j in range(2)]
    with Pool(min(16, len(jobs))) as pool:  # (before the device is opened: the workers are plain forks)
        flat = pool.map(render, jobs)
    imgs = [[np.ascontiguousarray(flat[2 * slot + j]) for j in range(2)] for slot in range(max(SIZES))]
    from lfvio import abi
    from lfvio.engine import Engine
    words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    cam = Engine.camera(tr.PAL)
    batch_eng = Engine(0)
    engines = [Engine(0) for _ in range(max(SIZES) if "turns" in ROUTES else 0)]
    cap = abi.TRACK_MAX_POINTS

    def buffers(n):
        outs, msgs, keep = (abi.TrackFrameOutC * n)(), (abi.TrackMessageC * n)(), []
        for i in range(n):
            a = dict(pts=np.zeros((cap, 2), np.float32), ids=np.zeros(cap, np.int32), track_cnt=np.zeros(cap, np.int32), un_pts=np.zeros((cap, 2), np.float32),
                     un_pts_3d=np.zeros((cap, 3), np.float32), velocity_3d=np.zeros((cap, 3), np.float32), rows=np.zeros((cap, 9), np.float32))
            for key, v in a.items():
                if key != "rows":
                    setattr(outs[i], key, v.ctypes.data_as(ip if v.dtype == np.int32 else fp))
            msgs[i].rows = a["rows"].ctypes.data_as(fp)
            keep.append(a)
        return outs, msgs, keep

    def entries(n):
        fin = (abi.TrackFrameInC * n)()
        for e in fin:
            e.width, e.height, e.publish, e.camera = W, H, 1, C.pointer(cam)
            e.win_size, e.max_level, e.max_iterations, e.epsilon, e.min_eig_threshold, e.border = 41, 3, 30, 0.01, 1e-4, 1
            e.max_count, e.quality_level, e.min_distance, e.mask_radius, e.num_samples, e.capacity = MAX_CNT, 0.01, MIN_DIST, MIN_DIST, S, cap
        return fin

    def point(fin, i):  # call i: the image walks back and forth, the words go round
        for slot, e in enumerate(fin):
            e.image, e.time = imgs[slot][i % 2].ctypes.data_as(up), 0.05 * i
            e.sample_words = words[(i + slot) % 8].ctypes.data_as(C.POINTER(C.c_uint))

    def tables(outs, keep):
        return b"".join(a[key][:outs[i].num_points].tobytes() for i, a in enumerate(keep) for key in ("pts", "ids", "track_cnt", "velocity_3d")), \
            [int(o.num_points) for o in outs]

    def run_batch(B, fin, outs, msgs, keep):
        lib, ctx = batch_eng.lib, batch_eng.ctx
        batch_eng.track_batch_reset(-1)
        ts = []
        for i in range(WARM + CALLS):
            point(fin, i)
            t = time.perf_counter(); rc = lib.lfvio_track_batch_frame(ctx, B, fin, outs, msgs); dt = time.perf_counter() - t
            assert rc == 0, rc
            if i >= WARM: ts.append(dt)
        return ts, tables(outs, keep)

    def run_turns(B, fin, outs, msgs, keep):
        lib = engines[0].lib
        call = lib.lfvio_track_frame_message
        ctxs = [e.ctx for e in engines[:B]]
        refs = [(C.byref(fin[s]), C.byref(outs[s]), C.byref(msgs[s])) for s in range(B)]
        for e in engines[:B]:
            e.track_frame_reset()
        ts = []
        for i in range(WARM + CALLS):
            point(fin, i)
            t = time.perf_counter()
            for s in range(B):
                rc = call(ctxs[s], refs[s][0], refs[s][1], None, refs[s][2])
                assert rc == 0, rc
            dt = time.perf_counter() - t
            if i >= WARM: ts.append(dt)
        return ts, tables(outs, keep)

    for B in SIZES:
        batch_eng.track_batch_reserve(B)
        fin = entries(B)
        res, last = {}, {}
        for _ in range(RUNS):  # (the routes alternate)
            for route in ROUTES:
                outs, msgs, keep = buffers(B)
                ts, last[route] = (run_batch if route == "batch" else run_turns)(B, fin, outs, msgs, keep)
                res.setdefault(route, []).append((float(np.median(ts)) * 1e6, float(np.percentile(ts, 95)) * 1e6))
        pts = next(iter(last.values()))[1]
        line = dict(size=f"{W}x{H}", max_cnt=MAX_CNT, samples=S, B=B, points_min=min(pts), points_max=max(pts))
        for route, v in res.items():
            line[route + "_median_us"], line[route + "_p95_us"] = [round(m) for m, _ in v], [round(p) for _, p in v]
            line[route + "_fps"] = round(B / (float(np.median([m for m, _ in v])) * 1e-6))
        if len(last) == 2:
            line["same_tables"] = last["batch"][0] == last["turns"][0]
            line["batch_below_turns"] = max(m for m, _ in res["batch"]) < min(m for m, _ in res["turns"])
            line["turns_over_batch"] = round(float(np.median([m for m, _ in res["turns"]]) / np.median([m for m, _ in res["batch"]])), 2)
        print(json.dumps(line), flush=True)
    batch_eng.track_batch_reserve(0)
    for e in engines + [batch_eng]:
        e.close()


if __name__ == "__main__":
    main()
