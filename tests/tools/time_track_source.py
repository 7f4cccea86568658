"""Tracking on the expanded image at the node's shape: 1280 x 960 bgr8 through the EQUIRECT map of the PAL camera into 960 x 480, MAX_CNT
150, MIN_DIST 30, S = 100, the LFVIO_CAM_EQUIRECT camera, lfvio_track_frame_message.  No pass / fail bar: one JSON line with median and
p95 per frame over 200 frames after 20 warm-up frames, three runs of each route on the same frames in the same process, the routes
alternating.  The frames are four klt_ref-rendered images of a slowly moving texture walked back and forth, as bgr8.
  source   the new route: lfvio_track_source_set on, the 1280 x 960 image goes up, level 0 is k_remap_gray's
  chain    (a) what there was before: lfvio_remap_apply (up, k_remap_apply, down), then the frame call on its output under {bgr8, step 0}
           (up again, k_img_gray); the SUM of the two calls' wall times
  plain    (b) the frame call alone on a 960 x 480 bgr8 image (the expanded one, made beforehand): what tracking costs without any expansion
`source` and `chain` get the same words and their last tables are compared.  The expectation DESIGN.md 3y states: source beats chain by
more than chain's own p95 - median spread, and stays within that spread of plain.
The kernels without the copies are not something a host clock sees: under `rocprofv3 --kernel-trace --stats -d <dir> -- python
tests/tools/time_track_source.py` with DBG_ROUTE=source (or chain) and DBG_FRAMES=50 read k_remap_gray<3> beside k_remap_apply<3> +
k_img_gray from the kernel statistics."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import image_ref as ir
import klt_ref as k
import project_ref as pr
from lfvio import abi
from lfvio.engine import Engine
eng = Engine(0)
SW, SH, W, H = 1280, 960, 960, 480
MAX_CNT, MIN_DIST, S, WARM = 150, 30, 100, 20
FRAMES, RUNS = int(os.environ.get("DBG_FRAMES", "200")), int(os.environ.get("DBG_RUNS", "3"))
ROUTES = os.environ.get("DBG_ROUTE", "source,chain,plain").split(",")
pal = pr.CAMS["PAL"][0]
cam = eng.camera(dict(model=abi.CAM_EQUIRECT, fx=float(W), fy=float(H)))
f = k.texture(7)
grey = [k.render(f, SW, SH, k.warp(SW, SH, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
src = [ir.from_gray(g, abi.IMG_BGR8, 0, seed=j) for j, g in enumerate(grey)]
walk = [0, 1, 2, 3, 2, 1]
words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST, width=W, height=H)
eng.remap_build(pal, abi.MAP_EQUIRECT, W, H, want_maps=False)
big = [eng.remap_apply(s, SW, SH, (W, H), encoding=abi.IMG_BGR8) for s in src]  # the expanded images, for `plain`
out = np.zeros((H, W * 3), np.uint8)

def run(route):
    eng.track_frame_reset()
    eng.image_format(abi.IMG_BGR8, 0)
    eng.track_source(SW, SH) if route == "source" else eng.track_source(None)
    ts, r = [], None
    for i in range(WARM + FRAMES):
        j, w = walk[i % 6], words[i % 8]
        t = time.perf_counter()
        if route == "source":
            r = eng.track_frame_message(src[j], 0.05 * i, cam, words=w, **KW)
        elif route == "chain":
            eng.remap_apply(src[j], SW, SH, (W, H), encoding=abi.IMG_BGR8, out=out)
            r = eng.track_frame_message(out, 0.05 * i, cam, words=w, **KW)
        else:
            r = eng.track_frame_message(big[j], 0.05 * i, cam, words=w, **KW)
        dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    return ts, (r["pts"].copy(), r["ids"].copy(), r["track_cnt"].copy(), r["velocity_3d"].copy(), r["rows"].copy())

res, last = {}, {}
for _ in range(RUNS):
    for route in ROUTES:
        ts, last[route] = run(route)
        res.setdefault(route, []).append((float(np.median(ts)) * 1e6, float(np.percentile(ts, 95)) * 1e6))
line = dict(shape=f"{SW}x{SH} bgr8 -> {W}x{H}", max_cnt=MAX_CNT, samples=S, frames=FRAMES, points=int(len(next(iter(last.values()))[1])))
for route, v in res.items():
    line[route + "_median_us"], line[route + "_p95_us"] = [round(m) for m, _ in v], [round(p) for _, p in v]
if "source" in last and "chain" in last:
    line["same_tables"] = all(a.tobytes() == b.tobytes() for a, b in zip(last["source"], last["chain"]))
    med = {r: float(np.median([m for m, _ in v])) for r, v in res.items()}
    spread = float(np.median([p - m for m, p in res["chain"]]))
    line["chain_minus_source_us"], line["chain_p95_minus_median_us"] = round(med["chain"] - med["source"]), round(spread)
    if "plain" in med:
        line["source_minus_plain_us"] = round(med["source"] - med["plain"])
line["gray_bytes"], line["chain_bytes"] = W * H * (4 + 3 + 1), W * H * ((4 + 2 * 3) + (3 + 1))
eng.track_source(None); eng.image_format(None)
eng.close()
print(json.dumps(line))
