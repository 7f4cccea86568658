"""Colour and 16-bit camera images at 1280 x 960, MAX_CNT 150, MIN_DIST 30, S = 100, the PAL camera: per encoding the median / p95
over 200 frames after 20 warm-up frames of three things, on the same frames in the same process —
  gray     lfvio_image_gray alone (one copy up, k_img_gray, one copy down: dominated by the copies)
  device   lfvio_track_frame_message on the raw image under lfvio_image_format_set (the device converts)
  host     the host function of csrc/image_format.h (imgfmt_to_gray, compiled with g++ -O2 behind ctypes) followed by the same call on grey
The claim to report is `device` against `host`.  The frames are those of tests/tools/time_track_frame.py made raw by
tests/image_ref.from_gray; both routes get the same words and their last tables are compared.  DBG_CODES=2,6 picks encodings."""
import ctypes as C, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import image_ref as ir
import klt_ref as k
import track_ref as tr
from lfvio.engine import Engine

SRC = '#include "image_format.h"\nextern "C" void to_gray(int code, int w, int h, long step, const unsigned char *s, unsigned char *d) { imgfmt_to_gray(code, w, h, (size_t)step, s, d); }\n'
d = tempfile.mkdtemp(prefix="time_image_format_")
open(os.path.join(d, "h.cpp"), "w").write(SRC)
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), os.path.join(d, "h.cpp"), "-o", os.path.join(d, "libh.so")])
host = C.CDLL(os.path.join(d, "libh.so"))
up = C.POINTER(C.c_ubyte)
host.to_gray.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, up, up]

eng = Engine(0)
W, H = [int(x) for x in os.environ.get("DBG_SIZE", "1280x960").split("x")]
MAX_CNT, MIN_DIST, S, FRAMES, WARM = int(os.environ.get("DBG_N", "150")), 30, 100, 200, 20
CODES = [int(x) for x in os.environ.get("DBG_CODES", "0,2,3,4,5,6,7").split(",")]
cam = eng.camera(tr.PAL)
f = k.texture(7)
grey = [k.render(f, W, H, k.warp(W, H, shift=(2.1 * j, -1.4 * j), angle=0.002 * j)[1]) for j in range(4)]
walk = [0, 1, 2, 3, 2, 1]
words = [np.random.default_rng([i, 5]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32) for i in range(8)]
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST, width=W, height=H)


def stats(ts):
    return round(float(np.median(ts)) * 1e6), round(float(np.percentile(ts, 95)) * 1e6)


def frames(convert, code, step, imgs):
    """convert None: the device converts (the format is set); otherwise the host function runs in front of every call."""
    eng.track_frame_reset()
    eng.image_format(code if convert is None else None, step)
    out, ts, r = np.zeros((H, W), np.uint8), [], None
    for i in range(WARM + FRAMES):
        img, w = imgs[walk[i % 6]], words[i % 8]
        t = time.perf_counter()
        if convert is not None:
            convert(code, W, H, step, img.ctypes.data_as(up), out.ctypes.data_as(up))
            r = eng.track_frame_message(out, 0.05 * i, cam, words=w, **KW)
        else:
            r = eng.track_frame_message(img, 0.05 * i, cam, words=w, **KW)
        dt = time.perf_counter() - t
        if i >= WARM:
            ts.append(dt)
    return ts, (r["pts"].tobytes(), r["ids"].tobytes(), r["track_cnt"].tobytes(), r["rows"].tobytes())


for code in CODES:
    step = W * ir.BPP[code] + (64 if code == 0 else 0)  # (mono8: padded rows, so that there is something to do)
    imgs = [ir.from_gray(g, code, step, seed=j) for j, g in enumerate(grey)]
    ts = []
    for i in range(WARM + FRAMES):
        t = time.perf_counter(); eng.image_gray(imgs[walk[i % 6]], W, H, code, step); dt = time.perf_counter() - t
        if i >= WARM:
            ts.append(dt)
    line = dict(size=f"{W}x{H}", code=code, name=ir.NAMES[code] + ("_be" if code == 7 else ""), step=step, max_cnt=MAX_CNT)
    line["gray_median_us"], line["gray_p95_us"] = stats(ts)
    td, last_d = frames(None, code, step, imgs)
    th, last_h = frames(host.to_gray, code, step, imgs)
    line["device_median_us"], line["device_p95_us"] = stats(td)
    line["host_median_us"], line["host_p95_us"] = stats(th)
    line["same_tables"] = last_d == last_h
    print(json.dumps(line), flush=True)
eng.image_format(None)
