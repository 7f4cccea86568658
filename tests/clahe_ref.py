"""Numpy restatement of lfvio_clahe_apply / lfvio_clahe_set (include/lfvio.h): cv::createCLAHE(clip_limit, Size(tiles_x,
tiles_y))->apply() on an 8-bit image, the equalize step of FeatureTracker::readImage (feature_tracker.cpp:101-107).  This file is the
SPECIFICATION of the device entries: it is written from the algorithm of OpenCV's 8-bit CLAHE_Impl::apply as stated
there; no OpenCV was at hand, so nobody has compared it with OpenCV itself.

  plan(w, h, clip_limit, tiles)        extent, tw, th, area, clip and the three float32 factors lut_scale, inv_tw, inv_th
  extended(img, tiles)                 the image continued right and down by (repeated) reflect-101 to the extent
  histograms(img, tiles)               [tiles_y, tiles_x, 256] int64 of the extended image's tiles
  luts(img, clip_limit, tiles)         [tiles_y, tiles_x, 256] uint8: clip, redistribute, cumulate, scale, round half to even
  interpolate(img, lut, tiles, fused)  the bilinear blend of the four tiles' LUTs, every float32 operation rounded on its own
                                       (fused=True: each product-sum pair as one fused multiply-add, what a contracting compiler emits)
  clahe(img, clip_limit, tiles)        (equalized image, luts)
  CASES / case_image(name)             the seeded cases tests/test_clahe.py runs on the device
"""
import numpy as np

import klt_ref as k

MAX_TILES, MAX_CLIP = 16, 1024.0  # LFVIO_CLAHE_MAX_TILES; the largest clip_limit
MIN_SIDE, MAX_SIDE = 16, 8192
F = np.float32


def extent(w, h, tiles, pad_both=True):
    """Both sides divide: the image's own size.  Otherwise each side grows by tiles - side % tiles, which is a whole `tiles` on a side
    that does divide (OpenCV's behaviour; pad_both=False is the variant that pads only the side that does not divide)."""
    tx, ty = tiles
    if w % tx == 0 and h % ty == 0:
        return w, h
    if not pad_both:
        return w + (tx - w % tx) % tx, h + (ty - h % ty) % ty
    return w + (tx - w % tx), h + (ty - h % ty)


def plan(w, h, clip_limit, tiles, pad_both=True):
    tx, ty = tiles
    ew, eh = extent(w, h, tiles, pad_both)
    tw, th = ew // tx, eh // ty
    area = tw * th
    clip = 0 if clip_limit == 0 else max(int(float(clip_limit) * float(area) / 256.0), 1)
    return dict(ext_w=ew, ext_h=eh, tw=tw, th=th, area=area, clip=clip, lut_scale=F(255.0) / F(area), inv_tw=F(1.0) / F(tw), inv_th=F(1.0) / F(th))


def extended(img, tiles, pad_both=True):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    ew, eh = extent(w, h, tiles, pad_both)
    return img[np.ix_(k.reflect101(np.arange(eh), h), k.reflect101(np.arange(ew), w))]


def histograms(img, tiles, pad_both=True):
    tx, ty = tiles
    ext = extended(img, tiles, pad_both)
    eh, ew = ext.shape
    tw, th = ew // tx, eh // ty
    tile = (np.arange(eh) // th)[:, None] * tx + (np.arange(ew) // tw)[None, :]
    return np.bincount((tile * 256 + ext).ravel(), minlength=tx * ty * 256).reshape(ty, tx, 256).astype(np.int64)


def redistribute(hist, clip):
    """hist [..., 256] int64 clipped at `clip` (> 0), the excess handed back: clipped / 256 to every bin, the rest one each to the bins
    0, step, 2 step, ... with step = max(256 / rest, 1).  Returns (hist, rest)."""
    clipped = np.maximum(hist - clip, 0).sum(axis=-1, keepdims=True)
    hist = np.minimum(hist, clip)
    batch = clipped // 256
    rest = clipped - 256 * batch
    hist = hist + batch
    step = np.maximum(256 // np.maximum(rest, 1), 1)
    i = np.arange(256)
    # rest * step <= 256: the loop `for (i = 0; i < 256 && rest > 0; i += step, rest--)` ends by rest, on the bins j * step, j < rest
    hist = hist + ((i % step == 0) & (i // step < rest))
    return hist, rest[..., 0]


def luts(img, clip_limit, tiles, pad_both=True):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    p = plan(img.shape[1], img.shape[0], clip_limit, tiles, pad_both)
    hist = histograms(img, tiles, pad_both)
    if p["clip"] > 0:
        hist, _ = redistribute(hist, p["clip"])
    scaled = np.cumsum(hist, axis=-1).astype(F) * p["lut_scale"]  # the integer sum to float, one multiply
    assert scaled.dtype == F
    return np.clip(np.rint(scaled), 0, 255).astype(np.uint8)


def axis_weights(n, inv, tiles):
    """Per pixel of an axis: (t1, t2 clamped tile indices, a, 1 - a) with t = x * inv - 0.5 in float32."""
    tf = np.arange(n).astype(F) * F(inv) - F(0.5)
    t1 = np.floor(tf)
    a = tf - t1
    a1 = F(1.0) - a
    assert tf.dtype == F and a.dtype == F and a1.dtype == F
    t1 = t1.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def interpolate(img, lut, tiles, fused=False, pad_both=True):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    p = plan(w, h, 1.0, tiles, pad_both)
    tx1, tx2, xa, xa1 = axis_weights(w, p["inv_tw"], tiles[0])
    ty1, ty2, ya, ya1 = axis_weights(h, p["inv_th"], tiles[1])
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    L = lambda ty, tx: lut[ty[:, None], tx[None, :], img].astype(F)
    a, b, c, d = L(ty1, tx1), L(ty1, tx2), L(ty2, tx1), L(ty2, tx2)
    if not fused:
        res = (a * xa1 + b * xa) * ya1 + (c * xa1 + d * xa) * ya
        assert res.dtype == F
    else:
        # fma(p, q, r) as float32(double(p) * double(q) + double(r)): the product of two float32 is exact in double
        D = np.float64
        fma = lambda p, q, r: (p.astype(D) * q.astype(D) + r.astype(D)).astype(F)
        top, bottom = fma(b, xa, a * xa1), fma(d, xa, c * xa1)
        res = fma(bottom, ya, top * ya1)
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(img, clip_limit=3.0, tiles=(8, 8), fused=False, pad_both=True):
    lut = luts(img, clip_limit, tiles, pad_both)
    return interpolate(img, lut, tiles, fused, pad_both), lut


# ---- the literal transcription: scalar loops over tiles, bins and pixels (tests/test_clahe_ref.py holds the functions above to it)
def clahe_loops(img, clip_limit, tiles):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    tx, ty = tiles
    if w % tx == 0 and h % ty == 0:
        ew, eh = w, h
    else:
        ew, eh = w + (tx - w % tx), h + (ty - h % ty)

    def reflect(i, n):
        while i < 0 or i >= n:
            i = -i if i < 0 else 2 * n - 2 - i
        return i
    tw, th = ew // tx, eh // ty
    area = tw * th
    clip = 0 if clip_limit == 0 else max(int(clip_limit * area / 256), 1)
    lut_scale = F(255.0) / F(area)
    lut = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            hist = [0] * 256
            for y in range(j * th, (j + 1) * th):
                for x in range(i * tw, (i + 1) * tw):
                    hist[int(img[reflect(y, h), reflect(x, w)])] += 1
            if clip > 0:
                clipped = 0
                for b in range(256):
                    if hist[b] > clip:
                        clipped += hist[b] - clip
                        hist[b] = clip
                batch = clipped // 256
                residual = clipped - 256 * batch
                for b in range(256):
                    hist[b] += batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    b = 0
                    while b < 256 and residual > 0:
                        hist[b] += 1
                        b += step
                        residual -= 1
            s = 0
            for b in range(256):
                s += hist[b]
                lut[j, i, b] = min(max(int(np.rint(F(s) * lut_scale)), 0), 255)
    out = np.zeros((h, w), np.uint8)
    inv_tw, inv_th = F(1.0) / F(tw), F(1.0) / F(th)
    for y in range(h):
        tyf = F(y) * inv_th - F(0.5)
        ty1 = int(np.floor(tyf))
        ya = tyf - F(ty1)
        ya1 = F(1.0) - ya
        ty2 = min(ty1 + 1, ty - 1)
        ty1 = max(ty1, 0)
        for x in range(w):
            txf = F(x) * inv_tw - F(0.5)
            tx1 = int(np.floor(txf))
            xa = txf - F(tx1)
            xa1 = F(1.0) - xa
            tx2 = min(tx1 + 1, tx - 1)
            tx1 = max(tx1, 0)
            v = int(img[y, x])
            res = (F(lut[ty1, tx1, v]) * xa1 + F(lut[ty1, tx2, v]) * xa) * ya1 + (F(lut[ty2, tx1, v]) * xa1 + F(lut[ty2, tx2, v]) * xa) * ya
            assert type(res) is F
            out[y, x] = min(max(int(np.rint(res)), 0), 255)
    return out, lut


# ---- test images
def textured(w, h, seed):
    return k.render(k.texture(seed), w, h)


def noise(w, h, seed):
    return np.random.default_rng([seed, 0x636c]).integers(0, 256, (h, w)).astype(np.uint8)


def two_valued(w, h, seed):
    """40 and 200 in blobs: every tile's histogram has at most two bins, both far above any clip."""
    return np.where(k.texture(seed)(*np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))) > 0, 200, 40).astype(np.uint8)


RESIDUALS = (1, 127, 129, 255)
RESIDUAL_CLIP = 12  # of 32 x 32 tiles with clip_limit 3.0


def residual_image(seed, batch):
    """64 x 64 for 2 x 2 tiles and clip_limit 3.0 (clip 12): in tile t the value 7 occurs 12 + 256 batch + RESIDUALS[t] times and
    every other value at most 12 times, so the clipped sum of tile t is 256 batch + RESIDUALS[t]."""
    rng = np.random.default_rng([seed, 0x726573])
    img = np.zeros((64, 64), np.uint8)
    for t, r in enumerate(RESIDUALS):
        n7 = RESIDUAL_CLIP + 256 * batch + r
        others = np.delete(np.arange(256), 7)
        rest = np.repeat(others, RESIDUAL_CLIP)[:1024 - n7]
        px = np.concatenate([np.full(n7, 7), rest])
        assert len(px) == 1024
        rng.shuffle(px)
        img[(t // 2) * 32:(t // 2) * 32 + 32, (t % 2) * 32:(t % 2) * 32 + 32] = px.reshape(32, 32)
    return img


# name -> (image kind, width, height, seed, clip_limit, tiles): what tests/test_clahe.py compares on the device, bit for bit
CASES = {
    "divides_64": ("tex", 64, 64, 0, 3.0, (8, 8)),          # both sides divide; tw = th = 8: dyadic weights
    "neither_97x75": ("tex", 97, 75, 0, 3.0, (8, 8)),      # ext 104 x 80
    "one_side_96x75": ("tex", 96, 75, 0, 3.0, (8, 8)),     # ext 104 x 80: the side that divides grows by a whole 8
    "tiny_tiles_16": ("noise", 16, 16, 1, 3.0, (8, 8)),     # 2 x 2 tiles, area 4, clip 1
    "repeated_16x31": ("noise", 16, 31, 2, 3.0, (16, 16)),  # ext 32 x 32: columns 16 .. 31 reflect to 14 .. 0, then 1
    "texture_345x339": ("tex", 345, 339, 0, 3.0, (8, 8)),
    "noise_640x480": ("noise", 640, 480, 0, 3.0, (8, 8)),
    "constant_64": ("const", 64, 64, 0, 3.0, (8, 8)),
    "two_valued_97x75": ("two", 97, 75, 3, 3.0, (8, 8)),
    "no_clip_97x75": ("tex", 97, 75, 1, 0.0, (8, 8)),
    "clip40_nothing_clipped": ("noise", 97, 75, 4, 40.0, (8, 8)),  # area 130, clip 20: no bin of a noise tile reaches it
    "tiles_1x1": ("tex", 64, 64, 2, 3.0, (1, 1)),               # one tile: every pixel blends one LUT with itself
    "tiles_3x5": ("tex", 97, 75, 2, 3.0, (3, 5)),            # ext 99 x 80: 75 divides by 5 and still grows
    "tiles_16x16": ("tex", 161, 123, 0, 3.0, (16, 16)),     # ext 176 x 128
    "residuals": ("res", 64, 64, 0, 3.0, (2, 2)),
    "residuals_batch": ("res1", 64, 64, 1, 3.0, (2, 2)),
    "track_161x123": ("tex", 161, 123, 0, 3.0, (8, 8)),
}
CONSTANT = 99


def case_image(name):
    kind, w, h, seed = CASES[name][:4]
    if kind == "tex":
        return textured(w, h, seed)
    if kind == "noise":
        return noise(w, h, seed)
    if kind == "const":
        return np.full((h, w), CONSTANT, np.uint8)
    if kind == "two":
        return two_valued(w, h, seed)
    return residual_image(seed, 0 if kind == "res" else 1)


def dyadic(name):
    """Both tile sides a power of two: every weight is a dyadic fraction, every product exact, and fusing changes nothing."""
    _, w, h, _, cl, tiles = CASES[name]
    p = plan(w, h, cl, tiles)
    return p["tw"] & (p["tw"] - 1) == 0 and p["th"] & (p["th"] - 1) == 0

