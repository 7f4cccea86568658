"""Numpy restatement of lfvio_gft_detect (include/lfvio.h): setMask and cv::goodFeaturesToTrack as FeatureTracker::readImage calls
them (feature_tracker/src/feature_tracker.cpp:46-83, :147-176).  This file is the SPECIFICATION of the device entry:
it follows OpenCV 3's featureselect.cpp / corner.cpp from knowledge of those files, no OpenCV was at hand to pin it.  Everything here
is exact integer arithmetic up to one correctly rounded float64 sqrt, so the device is held to it bit for bit.

  sobel(img)                         dx, dy: 3 x 3 Sobel on the image continued by reflect-101 (int64, |.| <= 1020)
  response(img)                      lambda = 0.5 (S - sqrt(D)), float64 [h, w]; OpenCV's value is lambda / (12 * 255)^2
  response_reflected_image(img)      the WRONG border rule (gradients of the reflected image), kept for the test that tells them apart
  round_half_even(v)                 cvRound
  set_mask(base, pts, cnt, r)        kept indices in kept order, their pixels, the final mask
  detect(img, mask, budget, q, d)    dict(corners [K, 2] float32, num_candidates, max_response)
  gft(img, base, pts, cnt, ...)      the whole call: dict(kept, corners, num_candidates, max_response, mask)
  annulus_mask(w, h, cx, cy, R, r)   255 where r^2 < dist^2 <= R^2 (Euclidean discs), as lfvio.engine.annulus_mask
  tiled(w, h, seed) / noise(...)     test images besides klt_ref's textures
"""
import numpy as np

import klt_ref as k

MAX_CORNERS, MAX_POINTS, MAX_RADIUS = 4096, 4096, 1024  # LFVIO_GFT_MAX_CORNERS, LFVIO_KLT_MAX_POINTS, the limit of both distances


def _sobel_inner(e):
    """The 3 x 3 Sobel responses on the interior of the int64 array e."""
    dx = (e[:-2, 2:] - e[:-2, :-2]) + 2 * (e[1:-1, 2:] - e[1:-1, :-2]) + (e[2:, 2:] - e[2:, :-2])
    dy = (e[2:, :-2] - e[:-2, :-2]) + 2 * (e[2:, 1:-1] - e[:-2, 1:-1]) + (e[2:, 2:] - e[:-2, 2:])
    return dx, dy


def sobel(img):
    return _sobel_inner(k.extend(np.asarray(img, dtype=np.uint8), 1).astype(np.int64))


def _box3(p):
    """3 x 3 box sum of the map p continued by reflect-101."""
    e = k.extend(p, 1)
    h, w = p.shape
    return sum(e[j:j + h, i:i + w] for j in range(3) for i in range(3))


def _lambda(a, b, c):
    S, D = a + c, (a - c) * (a - c) + 4 * b * b
    assert D.max(initial=0) < 2 ** 53
    return 0.5 * (S.astype(np.float64) - np.sqrt(D.astype(np.float64)))


def response(img):
    dx, dy = sobel(img)
    return _lambda(_box3(dx * dx), _box3(dx * dy), _box3(dy * dy))


def response_reflected_image(img):
    """NOT the specification: the image continued by a halo of 2 and differentiated there, then box sums without a border rule."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    dx, dy = _sobel_inner(k.extend(img, 2).astype(np.int64))  # gradients on [-1, w] x [-1, h]
    box = lambda p: sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3))
    return _lambda(box(dx * dx), box(dx * dy), box(dy * dy))


def round_half_even(v):
    return np.rint(np.asarray(v, dtype=np.float64))


def set_mask(base, pts, cnt, r):
    """Returns (kept [K] int32 indices into pts in kept order, pix [K, 2] int64 (x, y), mask uint8 [h, w])."""
    base = np.asarray(base, dtype=np.uint8)
    h, w = base.shape
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    cnt = np.asarray(cnt, dtype=np.int32).reshape(-1)
    order = sorted(range(len(pts)), key=lambda i: (-int(cnt[i]), i))
    kept, pix = [], np.zeros((len(pts), 2), np.int64)
    for i in order:
        x, y = pts[i]
        if np.isnan(x) or np.isnan(y):
            continue
        px, py = round_half_even(x), round_half_even(y)
        if not (0 <= px < w and 0 <= py < h):
            continue
        px, py = int(px), int(py)
        if base[py, px] != 255:
            continue
        q = pix[:len(kept)]
        if ((q[:, 0] - px) ** 2 + (q[:, 1] - py) ** 2 <= r * r).any():
            continue
        pix[len(kept)] = (px, py)
        kept.append(i)
    pix = pix[:len(kept)]
    mask = base.copy()
    for qx, qy in pix:  # (the disc's bounding box, cut to the image)
        xa, xb, ya, yb = max(qx - r, 0), min(qx + r, w - 1) + 1, max(qy - r, 0), min(qy + r, h - 1) + 1
        yy, xx = np.mgrid[ya:yb, xa:xb]
        mask[ya:yb, xa:xb][(xx - qx) ** 2 + (yy - qy) ** 2 <= r * r] = 0
    return np.array(kept, np.int32), pix, mask


def candidates(lam, mask, quality):
    """(flat pixel indices y * w + x of the candidates in pick order, max_response); no candidates where max_response is 0."""
    h, w = lam.shape
    open_ = mask != 0
    maxv = float(lam[open_].max()) if open_.any() else 0.0
    if maxv == 0.0:
        return np.zeros(0, np.int64), 0.0
    thr = np.float64(quality) * np.float64(maxv)
    e = np.full((h + 2, w + 2), -np.inf)
    e[1:-1, 1:-1] = lam
    nmax = np.max([e[1 + j:1 + j + h, 1 + i:1 + i + w] for j in (-1, 0, 1) for i in (-1, 0, 1)], axis=0)  # the UNMASKED map, dilated
    ok = (lam > thr) & (lam >= nmax) & open_
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    idx = np.flatnonzero(ok)
    return idx[np.lexsort((-idx, -lam.reshape(-1)[idx]))], maxv  # descending lambda, then the larger index first


def pick(idx, w, budget, d):
    """Greedy: accepted when every accepted corner is at squared distance >= d^2; stops at `budget`."""
    acc = np.zeros((0, 2), np.int64)
    out = []
    for p in idx:
        if len(out) >= budget:
            break
        x, y = int(p) % w, int(p) // w
        if d > 0 and len(out) and (((acc[:len(out), 0] - x) ** 2 + (acc[:len(out), 1] - y) ** 2) < d * d).any():
            continue
        if len(out) == len(acc):
            acc = np.concatenate([acc, np.zeros((max(64, len(acc)), 2), np.int64)])
        acc[len(out)] = (x, y)
        out.append((x, y))
    return np.array(out, np.float32).reshape(-1, 2)


def detect(img, mask, budget, quality, d, lam=None):
    none = dict(corners=np.zeros((0, 2), np.float32), num_candidates=0, max_response=0.0)
    if budget <= 0:
        return none
    lam = response(img) if lam is None else lam
    idx, maxv = candidates(lam, mask, quality)
    if maxv == 0.0:
        return none
    return dict(corners=pick(idx, lam.shape[1], budget, d), num_candidates=len(idx), max_response=maxv)


def gft(img, base=None, pts=None, cnt=None, max_count=150, quality=0.01, min_distance=30, mask_radius=30, lam=None):
    img = np.asarray(img, dtype=np.uint8)
    base = np.full(img.shape, 255, np.uint8) if base is None else np.asarray(base, dtype=np.uint8)
    pts = np.zeros((0, 2), np.float32) if pts is None else pts
    cnt = np.zeros(0, np.int32) if cnt is None else cnt
    kept, _, mask = set_mask(base, pts, cnt, mask_radius)
    r = detect(img, mask, max_count - len(kept), quality, min_distance, lam=lam)
    r.update(kept=kept, mask=mask)
    return r


def annulus_mask(w, h, cx, cy, max_r, min_r):
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    return np.where((d2 <= max_r * max_r) & (d2 > min_r * min_r), 255, 0).astype(np.uint8)


# ---- test images
def textured(w, h, seed):
    return k.render(k.texture(seed), w, h)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def tiled(w, h, seed):
    """One random 8 x 8 pattern repeated: every response value away from the border occurs once per tile."""
    pat = np.random.default_rng([seed, 0x746c]).integers(0, 256, (8, 8)).astype(np.uint8)
    return np.tile(pat, ((h + 7) // 8, (w + 7) // 8))[:h, :w].copy()


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def stripes(w, h, diagonal=False):
    """Stripes of two pixels, 0 / 255, vertical or diagonal: |dx| = 1020 on every pixel (and |dy| on the diagonal ones), the largest
    S and D.  (A checkerboard of single pixels has dx = dy = 0 everywhere: both Sobel taps of a row see the same grey value.)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((((xx + yy) if diagonal else xx) >> 1) & 1) * 255).astype(np.uint8)


def truth_image():
    img = np.full((48, 64), 20, np.uint8)
    img[10:30, 12:40] = 200
    return img


def tracked_case(w, h, seed, n=60):
    """n points with counts 1 .. 5, uniform in the image, on the grid of quarter pixels."""
    rng = np.random.default_rng([seed, 0x747261])
    pts = np.stack([rng.integers(0, 4 * (w - 1), n) / 4.0, rng.integers(0, 4 * (h - 1), n) / 4.0], axis=1).astype(np.float32)
    return pts, rng.integers(1, 6, n).astype(np.int32)
