"""The batched tracker on the expanded image (lfvio_track_batch_map / lfvio_track_batch_source) at the node's shape —
1280 x 960 bgr8 sources into a 960 x 480 equirectangular image through the PAL camera, MAX_CNT 150, MIN_DIST 30, S = 100,
lfvio_track_batch_frame with messages — for B = 1, 8, 64 streams, three routes that give the same tables:

  source  the new route: B source images up, one k_remap_gray_b, the launches of one frame
  turns   B contexts, each with its own map under lfvio_track_source_set, given their frame through lfvio_track_frame_message in turn
  apply   lfvio_remap_apply per stream (one copy up, one down each), then lfvio_track_batch_frame on the B expanded bgr8 images

Wall time per round at the C entry with every struct built beforehand, median and p95 over DBG_CALLS (100) rounds after 10 warm-up
rounds, DBG_RUNS (3) runs of each route, alternating; the last round's tables are compared.  One JSON line per B.

DBG_PLAIN=1 times the PLAIN batched frame instead (the setting off, 960 x 480 mono8, B = 8 and 64) on this build and, alternating with
it, on the library DBG_PARENT_LIB names (a build of the parent commit), a fresh child process per build and run: every run's median
and p95, and of the runs' medians both builds' median (this_us, parent_us), the parent's p95 - median spread, the bar (the parent's
median plus that spread) and whether this build is within it.

Clocks are the machine's defaults: nothing here sets one.  The date is printed with the results."""
import ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SW, SH, W, H = 1280, 960, 960, 480
MAX_CNT, MIN_DIST, S, WARM = 150, 30, 100, 10
CALLS, RUNS = int(os.environ.get("DBG_CALLS", "100")), int(os.environ.get("DBG_RUNS", "3"))
SIZES = [int(x) for x in os.environ.get("DBG_B", "1,8,64").split(",")]
ROUTES = os.environ.get("DBG_ROUTE", "source,turns,apply").split(",")
STREAMS = 8  # distinct image streams; slot s shows stream s % 8


def texture(seed, w, h):
    """A seeded grey image with corners everywhere: blocks of 16 x 16 pixels of random grey, smoothed a little."""
    rng = np.random.default_rng([seed, 77])
    g = np.kron(rng.integers(30, 226, (h // 16 + 2, w // 16 + 2)).astype(np.float32), np.ones((16, 16), np.float32))
    g = (g + np.roll(g, 1, 0) + np.roll(g, 1, 1) + np.roll(g, (1, 1), (0, 1))) / 4.0
    return g


def grey_pair(seed, w, h):
    """Two images of one texture, the second moved by (3, 2) pixels: every frame tracks a real flow, walked back and forth."""
    g = texture(seed, w + 16, h + 16)
    return [np.ascontiguousarray(g[8 + 2 * j:8 + 2 * j + h, 8 + 3 * j:8 + 3 * j + w].astype(np.uint8)) for j in range(2)]


def plain():
    """DBG_PLAIN: a fresh child process per build and run, the builds alternating; this process never opens the device."""
    import subprocess

    libs = {"this": ""}
    if os.environ.get("DBG_PARENT_LIB"):
        libs["parent"] = os.path.abspath(os.environ["DBG_PARENT_LIB"])
    print(json.dumps(dict(date=time.strftime("%Y-%m-%d"), clocks="defaults", plain=f"{W}x{H} mono8", max_cnt=MAX_CNT, samples=S, calls=CALLS, warm=WARM, runs=RUNS)),
          flush=True)
    res = {}
    for _ in range(RUNS):
        for name, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, DBG_PLAIN_CHILD=path), capture_output=True, text=True, timeout=240)
            if r.returncode != 0:  # nothing more is started on the device behind a child that failed
                print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
                sys.exit(r.returncode if r.returncode > 0 else 1)
            for ln in r.stdout.splitlines():
                if ln.startswith("{") and '"median_us"' in ln:
                    d = json.loads(ln)
                    res.setdefault(d["B"], {}).setdefault(name, []).append(d)
    for B, by in sorted(res.items()):
        line = dict(B=B, points=by["this"][-1]["points"])
        for name, v in by.items():
            line[name + "_median_us"], line[name + "_p95_us"] = [round(d["median_us"]) for d in v], [round(d["p95_us"]) for d in v]
        if "parent" in by:
            pm, pp = float(np.median([d["median_us"] for d in by["parent"]])), float(np.median([d["p95_us"] for d in by["parent"]]))
            tm = float(np.median([d["median_us"] for d in by["this"]]))
            line.update(same_tables=len({d["tables"] for v in by.values() for d in v}) == 1, parent_us=round(pm), parent_spread_us=round(pp - pm), this_us=round(tm),
                        bar_us=round(pm + (pp - pm)), within_bar=tm <= pm + (pp - pm))
        print(json.dumps(line), flush=True)


def main():
    if os.environ.get("DBG_PLAIN") and "DBG_PLAIN_CHILD" not in os.environ:
        return plain()
    from lfvio import abi
    from lfvio.engine import Engine
    import project_ref as pr

    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    cap = abi.TRACK_MAX_POINTS
    words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
    cam = Engine.camera(dict(model=abi.CAM_EQUIRECT, fx=float(W), fy=float(H)))
    print(json.dumps(dict(date=time.strftime("%Y-%m-%d"), clocks="defaults", source=f"{SW}x{SH} bgr8", tracked=f"{W}x{H}", max_cnt=MAX_CNT, samples=S,
                          calls=CALLS, warm=WARM, runs=RUNS)), flush=True)

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

    def point(fin, i, imgs):  # round i: the image walks back and forth, the words go round
        for slot, e in enumerate(fin):
            e.image, e.time = imgs[slot % STREAMS][i % 2].ctypes.data_as(up), 0.05 * i
            e.sample_words = words[(i + slot) % 8].ctypes.data_as(C.POINTER(C.c_uint))

    def tables(outs, keep):
        return b"".join(a[key][:outs[i].num_points].tobytes() for i, a in enumerate(keep) for key in ("pts", "ids", "track_cnt", "velocity_3d")), \
            [int(o.num_points) for o in outs]

    def stats(ts):
        return float(np.median(ts)) * 1e6, float(np.percentile(ts, 95)) * 1e6

    def batch_rounds(eng, B, fin, outs, msgs, keep, imgs, before=None):
        lib, ctx = eng.lib, eng.ctx
        eng.track_batch_reset(-1)
        ts = []
        for i in range(WARM + CALLS):
            point(fin, i, imgs)
            t = time.perf_counter()
            if before:
                before(fin, i)
            rc = lib.lfvio_track_batch_frame(ctx, B, fin, outs, msgs)
            dt = time.perf_counter() - t
            assert rc == 0, (rc, lib.lfvio_last_error(ctx))
            if i >= WARM:
                ts.append(dt)
        return ts, tables(outs, keep)

    if "DBG_PLAIN_CHILD" in os.environ:  # one build, one run: a JSON line per B with the median, the p95 and a digest of the tables
        import hashlib

        imgs = [grey_pair(200 + s, W, H) for s in range(STREAMS)]
        eng = Engine(0, lib_path=os.environ["DBG_PLAIN_CHILD"] or None)
        for B in [b for b in SIZES if b > 1]:
            eng.track_batch_reserve(B)
            outs, msgs, keep = buffers(B)
            ts, last = batch_rounds(eng, B, entries(B), outs, msgs, keep, imgs)
            m, p = stats(ts)
            print(json.dumps(dict(B=B, median_us=m, p95_us=p, points=last[1][:4], tables=hashlib.sha256(last[0]).hexdigest())), flush=True)
        eng.track_batch_reserve(0)
        eng.close()
        return

    pal = pr.PAL
    code, step = abi.IMG_BGR8, 3 * SW
    srcs = [[np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2).reshape(SH, step)) for g in grey_pair(100 + s, SW, SH)] for s in range(STREAMS)]
    batch_eng = Engine(0)
    engines = [Engine(0) for _ in range(max(SIZES) if "turns" in ROUTES else 0)]
    for e in engines:
        e.remap_build(pal, abi.MAP_EQUIRECT, W, H, want_maps=False)
        e.image_format(code, step)
        e.track_source(SW, SH)
    batch_eng.remap_build(pal, abi.MAP_EQUIRECT, W, H, want_maps=False)  # the apply route's map: the context's own
    expanded = [[np.zeros((H, 3 * W), np.uint8) for _ in range(2)] for _ in range(max(SIZES))]
    fmt = abi.ImageFormatC(code, step)

    def run_source(B, fin, outs, msgs, keep):
        batch_eng.track_batch_format(code, step)
        batch_eng.track_batch_source(SW, SH)
        batch_eng.track_batch_map(-1, pal, abi.MAP_EQUIRECT, W, H)
        return batch_rounds(batch_eng, B, fin, outs, msgs, keep, srcs)

    def run_apply(B, fin, outs, msgs, keep):
        batch_eng.track_batch_format(code, 0)
        batch_eng.track_batch_source(None)
        lib, ctx = batch_eng.lib, batch_eng.ctx

        def before(fin, i):  # every stream's image expanded by a call of its own, then handed to the batch
            for slot, e in enumerate(fin):
                dst = expanded[slot][i % 2]
                rc = lib.lfvio_remap_apply(ctx, C.byref(fmt), SW, SH, e.image, dst.ctypes.data_as(up))
                assert rc == 0, rc
                e.image = dst.ctypes.data_as(up)
        return batch_rounds(batch_eng, B, fin, outs, msgs, keep, srcs, before)

    def run_turns(B, fin, outs, msgs, keep):
        call = engines[0].lib.lfvio_track_frame_message
        ctxs = [e.ctx for e in engines[:B]]
        refs = [(C.byref(fin[s]), C.byref(outs[s]), C.byref(msgs[s])) for s in range(B)]
        for e in engines[:B]:
            e.track_frame_reset()
        ts = []
        for i in range(WARM + CALLS):
            point(fin, i, srcs)
            t = time.perf_counter()
            for s in range(B):
                rc = call(ctxs[s], refs[s][0], refs[s][1], None, refs[s][2])
                assert rc == 0, rc
            dt = time.perf_counter() - t
            if i >= WARM:
                ts.append(dt)
        return ts, tables(outs, keep)

    runs = dict(source=run_source, turns=run_turns, apply=run_apply)
    for B in SIZES:
        batch_eng.track_batch_reserve(B)
        fin, res, last = entries(B), {}, {}
        for _ in range(RUNS):  # (the routes alternate)
            for route in ROUTES:
                outs, msgs, keep = buffers(B)
                ts, last[route] = runs[route](B, fin, outs, msgs, keep)
                res.setdefault(route, []).append(stats(ts))
        pts = next(iter(last.values()))[1]
        line = dict(B=B, points_min=min(pts), points_max=max(pts), same_tables=len({v[0] for v in last.values()}) == 1)
        for route, v in res.items():
            line[route + "_median_us"], line[route + "_p95_us"] = [round(m) for m, _ in v], [round(p) for _, p in v]
            line[route + "_fps"] = round(B / (float(np.median([m for m, _ in v])) * 1e-6))
        print(json.dumps(line), flush=True)
    batch_eng.track_batch_source(None)
    batch_eng.track_batch_format(None)
    batch_eng.track_batch_reserve(0)
    for e in engines + [batch_eng]:
        e.close()


if __name__ == "__main__":
    main()
