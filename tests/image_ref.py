"""The specification of the image encodings of lfvio_image_format_set / lfvio_image_gray (include/lfvio.h) and of the type-10 record
(lf-vio_amd/host/replay.h), in numpy: what cv_bridge::toCvCopy(img_msg, MONO8) makes of a camera image in front of
FeatureTracker::readImage (feature_tracker/src/feature_tracker_node.cpp:64-78).

  code  name                    bytes / pixel  grey value
  0     mono8 (also 8UC1)       1              v
  2     bgr8                    3              (1868 B + 9617 G + 4899 R + 8192) >> 14
  3     rgb8                    3              the same on R, G, B in their places
  4     bgra8                   4              the same; the fourth byte is never read into the value
  5     rgba8                   4              the same
  6     mono16 (little endian)  2              (v + 128) // 257
  7     mono16, big endian      2              the same after the byte swap

The colour line is OpenCV 3.3's 8-bit RGB2Gray (14-bit coefficients, the rounding constant folded into its table); the 16-bit line is
cv_bridge's convertTo(..., CV_8U, 255. / 65535.), whose rounded float product equals the integer form for all 65 536 values
(gray_16_float below states it; test_image_format_ref.py compares the two).  Both are written down from memory of those libraries: no
OpenCV was at hand and nobody has compared them.  lf-vio_amd/csrc/image_format.h is the same text in C++ and
tests/test_image_format_ref.py holds it to this file."""
import numpy as np

MONO8, BGR8, RGB8, BGRA8, RGBA8, MONO16, MONO16_BE = 0, 2, 3, 4, 5, 6, 7
CODES = (MONO8, BGR8, RGB8, BGRA8, RGBA8, MONO16, MONO16_BE)
BPP = {MONO8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4, MONO16: 2, MONO16_BE: 2}
NAMES = {MONO8: "mono8", BGR8: "bgr8", RGB8: "rgb8", BGRA8: "bgra8", RGBA8: "rgba8", MONO16: "mono16", MONO16_BE: "mono16"}
MAX_STEP = 65536


def gray_bgr(b, g, r):
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def gray_bgr_float(b, g, r):
    """The formula the fixed-point line approximates, rounded half to even: NOT the specification (it differs on ~0.18 % of triples)."""
    b, g, r = (np.asarray(v).astype(np.float64) for v in (b, g, r))
    return np.clip(np.rint(0.114 * b + 0.587 * g + 0.299 * r), 0, 255).astype(np.uint8)


def gray_16(v):
    return ((np.asarray(v).astype(np.int64) + 128) // 257).astype(np.uint8)


def gray_16_float(v, dtype=np.float32):
    """convertTo(..., CV_8U, 255. / 65535.) as OpenCV computes it: the product in `dtype`, rounded half to even, saturated."""
    return np.clip(np.rint(np.asarray(v).astype(dtype) * dtype(255.0 / 65535.0)), 0, 255).astype(np.uint8)


def check(code, step, width):
    """None, or what is wrong (the refusals of imgfmt_check, image_format.h)."""
    if code not in BPP:
        return "encoding"
    if step < 0 or step > MAX_STEP:
        return "step range"
    if 0 < step < width * BPP[code]:
        return "step below the row"
    return None


def pixels(rows, width, code):
    """rows [height, step] uint8 -> the pixels' bytes [height, width, bytes per pixel]"""
    rows = np.asarray(rows, dtype=np.uint8)
    bpp = BPP[code]
    return rows[:, :width * bpp].reshape(rows.shape[0], width, bpp)


def to_gray(rows, width, code):
    """rows [height, step] uint8 in encoding `code` -> [height, width] uint8"""
    p = pixels(rows, width, code).astype(np.int64)
    if code == MONO8:
        return p[:, :, 0].astype(np.uint8)
    if code in (BGR8, BGRA8):
        return gray_bgr(p[:, :, 0], p[:, :, 1], p[:, :, 2])
    if code in (RGB8, RGBA8):
        return gray_bgr(p[:, :, 2], p[:, :, 1], p[:, :, 0])
    if code == MONO16:
        return gray_16(p[:, :, 0] | (p[:, :, 1] << 8))
    if code == MONO16_BE:
        return gray_16(p[:, :, 1] | (p[:, :, 0] << 8))
    raise ValueError(code)


def typed(rows, width, code):
    """rows -> what trace.read_trace returns for the record: [h, w] uint8, [h, w, C] uint8 or [h, w] uint16 (native values)"""
    p = pixels(rows, width, code)
    if code == MONO8:
        return p[:, :, 0].copy()
    if code in (MONO16, MONO16_BE):
        lo, hi = (0, 1) if code == MONO16 else (1, 0)
        return (p[:, :, lo].astype(np.uint16) | (p[:, :, hi].astype(np.uint16) << 8))
    return p.copy()


def pack(px, step, seed=None):
    """px [height, width, bpp] uint8 -> rows [height, step] uint8; the padding is seeded noise (seed None: zeros)."""
    h, w, bpp = px.shape
    step = w * bpp if not step else step
    assert step >= w * bpp
    rows = np.zeros((h, step), np.uint8) if seed is None else np.random.default_rng(seed).integers(0, 256, (h, step), dtype=np.uint8)
    rows[:, :w * bpp] = px.reshape(h, w * bpp)
    return rows


def from_gray(gray, code, step=0, seed=0):
    """A raw image in `code` made from the grey picture `gray` [h, w] uint8 so that its texture survives: colour = per-channel gains in
    0.6 .. 1.0 plus +-3 seeded noise, clipped, alpha random; 16 bits = g * 257 plus noise in +-128, clipped; mono8 = g.  The padding is
    noise.  Its grey twin is to_gray of the result, not `gray`.  -> rows [h, step] uint8"""
    rng = np.random.default_rng(seed)
    g = np.asarray(gray, dtype=np.uint8)
    h, w = g.shape
    bpp = BPP[code]
    if code == MONO8:
        px = g[:, :, None]
    elif code in (MONO16, MONO16_BE):
        v = np.clip(g.astype(np.int64) * 257 + rng.integers(-128, 129, (h, w)), 0, 65535)
        lo, hi = (v & 255).astype(np.uint8), (v >> 8).astype(np.uint8)
        px = np.stack([lo, hi] if code == MONO16 else [hi, lo], axis=2)
    else:
        gains = rng.uniform(0.6, 1.0, 3)
        ch = np.clip(np.rint(g[:, :, None] * gains[None, None, :]) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
        px = ch if bpp == 3 else np.concatenate([ch, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    return pack(px, step, seed=seed + 1000)
