"""Timing of lfvio_cloud_fuse at the reference node's shape: a 1280 x 960 bgr8 image through the EQUIRECT map of the PAL camera into
960 x 480 and a lidar scan of n = 131 072 points (an Ouster 128 x 1024) marked in it, point_step 48 and 12, through the node's pose.
No pass / fail bar: one JSON line with, over DBG_N calls (default 200) after 20 warm-up calls, the median and the p95 of the wall time of
  fuse_image        Engine.cloud_fuse, REMAP, paint on, only image_out brought down        (per point_step)
  fuse_all          the same with index, range and counts as well                          (per point_step)
  fuse_points       no image: index, range and counts                                      (per point_step)
  apply             Engine.remap_apply alone
  apply_host        Engine.remap_apply followed by the overlay on the host: fuse_ref.points on the cloud's fields and the paint in numpy,
                    what a node without the fused call would do
Set DBG_LIB to a library's path below lf-vio_amd/ to time another build; the fused calls are skipped where it lacks the symbol.
The three kernels WITHOUT the copies are not something a host clock sees: run the same script under `rocprofv3 --kernel-trace --stats
-d <dir> -- python tests/tools/time_fuse.py` (DBG_N=50 is enough) and read k_fuse_project, k_fuse_sample and k_fuse_paint from the
kernel statistics (k_fuse_sample runs only where colour is asked for: DBG_COLOUR=1 adds it to fuse_all)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fuse_ref as fr
import project_ref as pr
from lfvio import abi
from lfvio.engine import Engine
LIB = os.environ.get("DBG_LIB")
eng = Engine(0, os.path.join(ROOT, "lf-vio_amd", LIB)) if LIB else Engine(0)
N, WARM = int(os.environ.get("DBG_N", "200")), 20
COLOUR = bool(int(os.environ.get("DBG_COLOUR", "0")))
SW, SH, W, H, POINTS = 1280, 960, 960, 480, 131072
PAINT = (255, 0, 0)
cam = pr.CAMS["PAL"][0]
src = pr.noise_image(1, SW, SH, abi.IMG_BGR8)
out = np.zeros((H, W * 3), np.uint8)
P = fr.sphere_cloud(POINTS, seed=1)
v = fr.view(width=W, height=H, R=fr.node_R(), T=fr.NODE_T, min_range=0.5, max_range=100.0)

def stats(f):
    ts = []
    for i in range(WARM + N):
        t = time.perf_counter(); f(); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    ts = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p95_ms=round(float(np.percentile(ts, 95)), 4))

res = dict(shape=f"{SW}x{SH} bgr8 -> {W}x{H}, n = {POINTS}", calls=N, lib=LIB or "liblfvio_hip.so")
mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
flat = pr.remap(src, mx, my, SW, SH, abi.IMG_BGR8)
res["apply"] = stats(lambda: eng.remap_apply(src, SW, SH, (W, H), encoding=abi.IMG_BGR8, out=out))
assert np.array_equal(out, flat)
want = fr.fuse(v, P[:, 0], P[:, 1], P[:, 2], image=flat, bpp=3, paint=PAINT)

def host_overlay(data, step):
    img = eng.remap_apply(src, SW, SH, (W, H), encoding=abi.IMG_BGR8, out=out)
    index = fr.points(v, *fr.fields(data, POINTS, step, 0, 4, 8))[0]
    img.reshape(-1, 3)[index[index >= 0]] = PAINT
    return img

if hasattr(eng.lib, "lfvio_cloud_fuse"):
    for step in (48, 12):
        data = fr.pack_cloud(P, step, (0, 4, 8), seed=step)
        kw = dict(R=v["R"], T=v["T"], min_range=v["min_range"], max_range=v["max_range"])
        img_kw = dict(kw, image=src, image_mode=abi.FUSE_IMAGE_REMAP, src_size=(SW, SH), encoding=abi.IMG_BGR8, paint=PAINT)
        bufs = dict(index=np.zeros(POINTS, np.int32), range=np.zeros((H, W), np.float32), counts=np.zeros(3, np.int32), image_out=np.zeros((H, W * 3), np.uint8),
                    colour=np.zeros((POINTS, 3), np.uint8))
        pick = lambda *names: {k: bufs[k] for k in names}
        every = ("index", "range", "counts", "image_out") + (("colour",) if COLOUR else ())
        res[f"fuse_image_{step}"] = stats(lambda: eng.cloud_fuse(data, POINTS, step, (0, 4, 8), W, H, want=(), out=pick("image_out"), **img_kw))
        assert np.array_equal(bufs["image_out"], want["image_out"])
        res[f"fuse_all_{step}"] = stats(lambda: eng.cloud_fuse(data, POINTS, step, (0, 4, 8), W, H, want=(), out=pick(*every), **img_kw))
        assert all(np.array_equal(bufs[k], want[k]) for k in every)
        res[f"fuse_points_{step}"] = stats(lambda: eng.cloud_fuse(data, POINTS, step, (0, 4, 8), W, H, want=(), out=pick("index", "range", "counts"), **kw))
        assert np.array_equal(bufs["index"], want["index"]) and bufs["range"].tobytes() == want["range"].tobytes()
    res["kept"] = int(want["counts"][0])
    res["pixels_marked"] = int(np.isfinite(want["range"]).sum())
    WARM, N = 2, max(N // 10, 5)  # (the numpy overlay takes tens of milliseconds)
    data = fr.pack_cloud(P, 48, (0, 4, 8), seed=48)
    res["apply_host_48"] = stats(lambda: host_overlay(data, 48))
    assert np.array_equal(out, want["image_out"])
eng.close()
print(json.dumps(res))
