"""Timing of the remap calls at the reference node's shape: a 1280 x 960 bgr8 image through the EQUIRECT map of the PAL camera into
960 x 480 (pointcloud_image_fusion_node.cpp:62-81).  No pass / fail bar: one JSON line with, over DBG_N calls (default 200) after
20 warm-up calls, the median and the p95 of the wall time of
  apply        Engine.remap_apply: the image up, k_remap_apply, the output down, the wait for it (the call WITH its copies)
  build        Engine.remap_build with both maps returned (k_remap_build, two copies down, the wait)
  project      Engine.cam_project at n = 1000
and
  copy_gbps    a device-to-device copy of 256 MiB on the same device in the same process (torch, device events; read + written
               bytes over time): the rate the apply kernel's bytes are set against
  apply_bytes  what k_remap_apply moves by its shape: per output pixel 4 bytes of integer map, 3 gathered, 3 written.
The kernel WITHOUT the copies is not something a host clock sees: run the same script under `rocprofv3 --kernel-trace --stats -d
<dir> -- python tests/tools/time_remap.py` (DBG_N=50 is enough) and read k_remap_apply<3>, k_remap_build and k_cam_project from
the kernel statistics; apply_bytes over that time, over copy_gbps, is the fraction DESIGN.md 3w reports."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import project_ref as pr
from lfvio import abi
from lfvio.engine import Engine
eng = Engine(0)
N, WARM = int(os.environ.get("DBG_N", "200")), 20
SW, SH, W, H = 1280, 960, 960, 480
cam = pr.CAMS["PAL"][0]
src = pr.noise_image(1, SW, SH, abi.IMG_BGR8)
out = np.zeros((H, W * 3), np.uint8)
rays = pr.sphere_rays("PAL", 1000)

def stats(f):
    ts = []
    for i in range(WARM + N):
        t = time.perf_counter(); f(); dt = time.perf_counter() - t
        if i >= WARM: ts.append(dt)
    ts = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p95_ms=round(float(np.percentile(ts, 95)), 4))

res = dict(shape=f"{SW}x{SH} bgr8 -> {W}x{H}", calls=N)
res["build"] = stats(lambda: eng.remap_build(cam, abi.MAP_EQUIRECT, W, H))
mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
res["apply"] = stats(lambda: eng.remap_apply(src, SW, SH, (W, H), encoding=abi.IMG_BGR8, out=out))
assert np.array_equal(out, pr.remap(src, mx, my, SW, SH, abi.IMG_BGR8))
res["project"] = stats(lambda: eng.cam_project(cam, rays))
res["apply_bytes"] = W * H * (4 + 3 + 3)
res["inside_share"] = round(float((pr.offsets(mx, my, SW, SH, SW * 3, 3) >= 0).mean()), 4)

import torch
a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0"); b = torch.empty_like(a)
for _ in range(3): b.copy_(a)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): b.copy_(a)
e1.record(); torch.cuda.synchronize()
res["copy_gbps"] = round(20 * 2 * a.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
eng.close()
print(json.dumps(res))
