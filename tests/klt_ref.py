"""Float64 numpy restatement of lfvio_klt_track (include/lfvio.h): the pyramidal Lucas-Kanade tracker of
cv::calcOpticalFlowPyrLK as feature_tracker.cpp:127 calls it, plus the inBorder test of :6-12 and :129-131.  This file is the
SPECIFICATION of the device entry: it follows OpenCV 3's lkpyramid.cpp from knowledge of that file, no OpenCV was
at hand to pin it, and where OpenCV interpolates in fixed point (14-bit weights, 5 fractional bits in the patch) this file and the
device use plain floating point.

  plan(w, h, win, max_level)          level sizes, levels_used and the byte offsets of the levels in a pyramid buffer
  pyr_down(img) / pyramid(img, ...)   [1 4 6 4 1]/16 twice, reflect-101, even pixels, (s + 128) >> 8: exact in uint8
  reflect101(i, n)                    the border rule, with repeated reflection
  track(prev_pyr, next_pyr, pts, ...) dict(next [N, 2] float32, status [N] uint8, iterations [N, max_level + 1] int32,
                                      levels_used, num_tracked, min_eig [N] of level 0)
  texture(seed) / render(...)         the seeded analytic test images of tests/test_klt_ref.py, tests/test_klt.py
"""
import numpy as np

MAX_POINTS, MAX_LEVEL = 4096, 5  # LFVIO_KLT_MAX_POINTS, LFVIO_KLT_MAX_LEVEL
FLT_EPSILON = float(np.finfo(np.float32).eps)
ALIGN = 256  # of a level's offset in the pyramid buffer (klt_plan.h)


def plan(w, h, win, max_level):
    """Level k + 1 is ((w_k + 1) / 2, (h_k + 1) / 2); building stops before the first level whose width or height is <= win and
    behind max_level.  Returns dict(sizes [(w, h)] of levels 0 .. levels_used, levels_used, offsets, bytes)."""
    sizes = [(w, h)]
    while len(sizes) <= max_level:
        nw, nh = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= win or nh <= win:
            break
        sizes.append((nw, nh))
    offsets, end = [], 0
    for lw, lh in sizes:
        offsets.append(end)
        end = (end + lw * lh + ALIGN - 1) // ALIGN * ALIGN
    return dict(sizes=sizes, levels_used=len(sizes) - 1, offsets=offsets, bytes=end)


def reflect101(i, n):
    """Index i of an axis of length n >= 2 continued by reflection about the centres of its end pixels (... 2 1 | 0 1 2 ...),
    again and again where one reflection does not reach the axis.  Arrays or scalars."""
    p = 2 * n - 2
    m = np.mod(np.asarray(i, dtype=np.int64), p)
    return np.where(m >= n, p - m, m)


def pyr_down(img):
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    ow, oh = (w + 1) // 2, (h + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    hor = sum(k[t] * src[:, reflect101(2 * np.arange(ow) - 2 + t, w)] for t in range(5))
    ver = sum(k[t] * hor[reflect101(2 * np.arange(oh) - 2 + t, h), :] for t in range(5))
    return ((ver + 128) >> 8).astype(np.uint8)


def pyramid(img, win, max_level):
    """Levels 0 .. levels_used of plan()."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    p = plan(img.shape[1], img.shape[0], win, max_level)
    levels = [img]
    for _ in range(p["levels_used"]):
        levels.append(pyr_down(levels[-1]))
    assert [(l.shape[1], l.shape[0]) for l in levels] == p["sizes"]
    return levels


def extend(img, pad):
    """img continued by `pad` pixels on every side by reflect101."""
    h, w = img.shape
    return img[np.ix_(reflect101(np.arange(-pad, h + pad), h), reflect101(np.arange(-pad, w + pad), w))]


def gradients(img):
    """Scharr 3 / 10 / 3 over 32 on the uint8 level, reflect-101 neighbours at the edge: grey levels per pixel, float64 (exact)."""
    e = extend(img, 1).astype(np.int64)
    gx = 3 * (e[:-2, 2:] - e[:-2, :-2]) + 10 * (e[1:-1, 2:] - e[1:-1, :-2]) + 3 * (e[2:, 2:] - e[2:, :-2])
    gy = 3 * (e[2:, :-2] - e[:-2, :-2]) + 10 * (e[2:, 1:-1] - e[:-2, 1:-1]) + 3 * (e[2:, 2:] - e[:-2, 2:])
    return gx / 32.0, gy / 32.0


def _bilinear(tap, ix, iy, a, b, win):
    """The win x win patch at corner (ix + a, iy + b): tap(xs, ys) gives the pixels of the columns xs and rows ys."""
    v = tap(ix + np.arange(win + 1), iy + np.arange(win + 1))
    return (1 - a) * (1 - b) * v[:-1, :-1] + a * (1 - b) * v[:-1, 1:] + (1 - a) * b * v[1:, :-1] + a * b * v[1:, 1:]


def _image_tap(img):
    h, w = img.shape
    return lambda xs, ys: img[np.ix_(reflect101(ys, h), reflect101(xs, w))].astype(np.float64)


def _zero_tap(g):
    """Outside the level a derivative is 0."""
    h, w = g.shape

    def tap(xs, ys):
        out = np.zeros((len(ys), len(xs)))
        my, mx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
        out[np.ix_(my, mx)] = g[np.ix_(ys[my], xs[mx])]
        return out
    return tap


def _outside(fx, fy, win, cols, rows):
    """The bounds test of a window's corner, on its floor (NaN is outside)."""
    return not (fx >= -win and fx < cols and fy >= -win and fy < rows)


def track(prev_pyr, next_pyr, pts, win=41, max_level=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, border=1, dtype=np.float64):
    """prev_pyr, next_pyr: pyramid() of the two images with the same win and max_level.  dtype: the arithmetic (float32 for the
    precision comparison of DESIGN.md 3k; the specification is float64)."""
    T = dtype
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
    N, LU = len(pts), len(prev_pyr) - 1
    rows0, cols0 = prev_pyr[0].shape
    grads = [gradients(l) for l in prev_pyr]
    taps = [(_image_tap(prev_pyr[L]), _zero_tap(grads[L][0]), _zero_tap(grads[L][1]), _image_tap(next_pyr[L])) for L in range(LU + 1)]
    nxt = np.zeros((N, 2), np.float32)
    status = np.ones(N, np.uint8)
    iters = np.zeros((N, max_level + 1), np.int32)
    min_eig = np.full(N, np.nan)
    half = T((win - 1) * 0.5)
    for n in range(N):
        p = pts[n].astype(T)
        guess = None
        for L in range(LU, -1, -1):
            rows, cols = prev_pyr[L].shape
            tapI, tapX, tapY, tapJ = taps[L]
            prev = p / T(1 << L)
            guess = prev.copy() if L == LU else guess * T(2)
            corner = prev - half
            f = np.floor(corner)
            if _outside(f[0], f[1], win, cols, rows):
                if L == 0:
                    status[n] = 0
                continue
            ix, iy = int(f[0]), int(f[1])
            a, b = T(corner[0] - f[0]), T(corner[1] - f[1])
            Ip, gx, gy = (_bilinear(t, ix, iy, a, b, win).astype(T) for t in (tapI, tapX, tapY))
            A11, A12, A22 = (gx * gx).sum(dtype=T) / T(1024), (gx * gy).sum(dtype=T) / T(1024), (gy * gy).sum(dtype=T) / T(1024)
            det = A11 * A22 - A12 * A12
            me = (A11 + A22 - np.sqrt((A11 - A22) * (A11 - A22) + T(4) * A12 * A12)) / T(2 * win * win)
            if L == 0:
                min_eig[n] = me
            if me < min_eig_threshold or det < FLT_EPSILON:
                if L == 0:
                    status[n] = 0
                continue
            prev_delta = None
            for j in range(max_iterations):
                corner = guess - half
                f = np.floor(corner)
                if _outside(f[0], f[1], win, cols, rows):
                    if L == 0:
                        status[n] = 0
                    break
                Jp = _bilinear(tapJ, int(f[0]), int(f[1]), T(corner[0] - f[0]), T(corner[1] - f[1]), win).astype(T)
                d = Jp - Ip
                b1, b2 = (d * gx).sum(dtype=T) / T(1024), (d * gy).sum(dtype=T) / T(1024)
                delta = np.array([(A12 * b2 - A22 * b1) / det, (A12 * b1 - A11 * b2) / det], dtype=T)
                guess = guess + delta
                iters[n, L] = j + 1
                if delta @ delta <= T(epsilon) * T(epsilon):
                    break
                if j > 0 and abs(delta[0] + prev_delta[0]) < 0.01 and abs(delta[1] + prev_delta[1]) < 0.01:
                    guess = guess - delta * T(0.5)
                    break
                prev_delta = delta
        nxt[n] = guess.astype(np.float32)
        if status[n] and border >= 0:
            x, y = np.rint(nxt[n].astype(np.float64))  # half to even, like cvRound
            if not (border <= x < cols0 - border and border <= y < rows0 - border):
                status[n] = 0
    return dict(next=nxt, status=status, iterations=iters, levels_used=LU, num_tracked=int(status.sum()), min_eig=min_eig)


# ---- seeded test images: an analytic texture rendered at analytically warped coordinates, so the true flow is known exactly

def texture(seed, count=60):
    """f(x, y) = sum of `count` sinusoids of random direction and phase, wavelength uniform in 8 .. 80 px, amplitude proportional
    to the wavelength; scaled to a standard deviation of 35 (the variance of the sum is half the sum of the squared amplitudes)."""
    rng = np.random.default_rng([seed, 0x4b4c54])
    lam = rng.uniform(8.0, 80.0, count)
    ang = rng.uniform(0.0, 2 * np.pi, count)
    ph = rng.uniform(0.0, 2 * np.pi, count)
    amp = lam * (35.0 / np.sqrt(0.5 * (lam * lam).sum()))
    kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)

    def f(x, y):
        out = np.zeros(np.broadcast(x, y).shape)
        for k in range(count):
            out += amp[k] * np.sin(kx[k] * x + ky[k] * y + ph[k])
        return out
    return f


def warp(w, h, shift=(0.0, 0.0), scale=0.0, angle=0.0):
    """W(p) = c + (1 + scale) R(angle) (p - c) + shift about the image centre c: (forward on [N, 2] points, inverse on x, y grids)."""
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    M = (1.0 + scale) * np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    Mi, s = np.linalg.inv(M), np.asarray(shift, dtype=np.float64)

    def fwd(p):
        return (np.asarray(p, dtype=np.float64) - c) @ M.T + c + s

    def inv(x, y):
        dx, dy = x - c[0] - s[0], y - c[1] - s[1]
        return Mi[0, 0] * dx + Mi[0, 1] * dy + c[0], Mi[1, 0] * dx + Mi[1, 1] * dy + c[1]
    return fwd, inv


def render(f, w, h, inv=None):
    """127.5 + f, at inv(pixel) for the second image, rounded to uint8."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    if inv is not None:
        x, y = inv(x, y)
    return np.clip(np.rint(127.5 + f(x, y)), 0, 255).astype(np.uint8)


# case -> (width, height, win, shift, scale, angle, levels used, points); max_level is 3 everywhere (the reference's)
CASES = {
    "a": (345, 339, 41, (17.4, 11.8), 0.0, 0.0, 3, 65),
    "b": (345, 339, 41, (3.2, -2.1), 0.02, 0.02, 3, 24),
    "c": (161, 123, 41, (6.3, -4.7), 0.0, 0.0, 1, 24),
    "d1": (177, 185, 21, (9.5, -7.25), 0.0, 0.0, 3, 24),
    "d2": (177, 185, 21, (0.37, -0.81), 0.0, 0.0, 3, 24),
    "e": (97, 75, 21, (1.5, 2.25), 0.01, 0.01, 1, 24),
}
PURE_SHIFTS = ("a", "c", "d1", "d2")


def make_case(name, seed):
    """dict(img0, img1, pts float32 [N, 2], true [N, 2] float64 (where the points of img0 are in img1), win, levels_used)."""
    w, h, win, shift, scale, angle, lu, n = CASES[name]
    f = texture(seed)
    fwd, inv = warp(w, h, shift, scale, angle)
    margin = (win - 1) // 2 + 4 + int(np.ceil(np.hypot(*shift)))
    rng = np.random.default_rng([seed, sorted(CASES).index(name), 0x707473])
    pts = np.stack([rng.uniform(margin, w - 1 - margin, n), rng.uniform(margin, h - 1 - margin, n)], axis=1).astype(np.float32)
    return dict(img0=render(f, w, h), img1=render(f, w, h, inv), pts=pts, true=fwd(pts), win=win, levels_used=lu)


STATUS_POINTS = np.array([[30, 150], [46, 150], [49, 150], [-50, 10], [200, 150], [60, 100], [200, 2.6], [120.5, 1.75], [300, 3]], np.float32)
STATUS_WANT = np.array([0, 0, 0, 0, 1, 1, 0, 0, 0], np.uint8)  # with border = 1; the last three are tracked to row 0 or -1: 1 with border = -1


def make_status_case():
    """Case (a)'s shape, a pure shift up and to the left, both images one grey value for x < 70.  STATUS_POINTS: two windows in the
    flat part (minEig 0) and one reaching a sliver of texture (minEig 6e-6 < 1e-4), a point whose level-0 window starts left of
    -win, two textured points, three points tracked out of the border."""
    w, h, win = CASES["a"][:3]
    f = texture(0)
    fwd, inv = warp(w, h, (-3.25, -2.5))
    img0, img1 = render(f, w, h), render(f, w, h, inv)
    img0[:, :70] = 128
    img1[:, :70] = 128
    return dict(img0=img0, img1=img1, pts=STATUS_POINTS.copy(), true=fwd(STATUS_POINTS), win=win, levels_used=3)


def run_case(c, **kw):
    a, b = pyramid(c["img0"], c["win"], 3), pyramid(c["img1"], c["win"], 3)
    return track(a, b, c["pts"], win=c["win"], max_level=3, **kw)
