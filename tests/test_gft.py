"""lfvio_gft_detect / lfvio_gft_set_mask / lfvio_gft_response (kernels_gft.h) against the numpy restatement tests/gft_ref.py, which
is the specification (tests/test_gft_ref.py holds it to its fixture).  Everything is compared bit for bit: no tolerance, nothing
excluded.  Images are rendered from seeds; the shapes are the smallest that reach each path.

  1  the response equals the restatement's bits (this is also the check that sqrt(double) is correctly rounded on the device);
  2  kept, corners, their order, num_candidates and max_response on textures, and on 640 x 480 noise whose candidates exceed what one
     workgroup's LDS holds;
  3  plateaus and ties: an image tiled with one 8 x 8 pattern;
  4  the base mask: annulus, value 128, kept points and their discs, all zero, no budget, N = 0, another size;
  5  repeatability; the resident pyramid is not written; the base mask survives lfvio_klt_reset;
  6  argument errors leave the outputs untouched;
  7  beside an optimization in flight."""
import functools

import numpy as np
import pytest

import gft_ref as g
import klt_ref as k

pytestmark = pytest.mark.gpu
NO_POINTS = np.zeros((0, 2), np.float32)
NO_COUNTS = np.zeros(0, np.int32)


@functools.lru_cache(maxsize=None)
def image(kind, w, h, seed=0):
    if kind in ("checker", "stripes", "diagonal"):
        img = g.checkerboard(w, h) if kind == "checker" else g.stripes(w, h, kind == "diagonal")
    else:
        img = dict(tex=g.textured, noise=g.noise, tiled=g.tiled)[kind](w, h, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def lam_of(kind, w, h, seed=0):
    lam = g.response(image(kind, w, h, seed))
    lam.setflags(write=False)
    return lam


def resident(eng, img):
    """img made resident without tracking (N = 0)."""
    r = eng.klt_track(img, NO_POINTS, want_iterations=False)
    assert r["rc"] == 0


def same(got, want):
    """kept, corners and their order, num_candidates, max_response: exactly."""
    assert got["rc"] == 0
    assert np.array_equal(got["kept"], want["kept"]), (got["kept"], want["kept"])
    assert got["num_candidates"] == want["num_candidates"], (got["num_candidates"], want["num_candidates"])
    assert np.float64(got["max_response"]).tobytes() == np.float64(want["max_response"]).tobytes(), (got["max_response"], want["max_response"])
    assert got["corners"].shape == want["corners"].shape, (got["corners"].shape, want["corners"].shape)
    assert got["corners"].tobytes() == want["corners"].tobytes()


def same_bits(a, b):
    return (a["kept"].tobytes() == b["kept"].tobytes() and a["corners"].tobytes() == b["corners"].tobytes()
            and (a["num_candidates"], a["rc"]) == (b["num_candidates"], b["rc"]) and np.float64(a["max_response"]).tobytes() == np.float64(b["max_response"]).tobytes())


# (the checkerboard of single pixels has dx = dy = 0 on every pixel, so its response is all zeros; the stripes of two pixels reach
# |dx| = 1020 everywhere: the largest S and D)
RESPONSE_IMAGES = [("noise", 16, 16, 3), ("tex", 97, 75, 0), ("tex", 345, 339, 0), ("noise", 161, 123, 1), ("checker", 33, 31, 0), ("stripes", 35, 33, 0),
                   ("diagonal", 35, 33, 0)]


@pytest.mark.parametrize("kind,w,h,seed", RESPONSE_IMAGES)
def test_response(eng, kind, w, h, seed):
    img = image(kind, w, h, seed)
    resident(eng, img)
    got, want = eng.gft_response(), lam_of(kind, w, h, seed)
    assert got.dtype == np.float64 and got.shape == want.shape
    differ = got.view(np.uint64) != want.view(np.uint64)
    print(f"{kind} {w} x {h}: {int(differ.sum())} of {differ.size} values differ, max lambda {want.max():.6g}")
    assert not differ.any(), np.argwhere(differ)[:8]


def test_response_of_a_constant_image_and_without_an_image(eng):
    eng.klt_reset()
    assert eng.gft_response(check=False) is None
    resident(eng, np.full((40, 56), 99, np.uint8))
    got = eng.gft_response()
    assert got.shape == (40, 56) and not got.view(np.uint64).any()
    r = eng.gft_detect(NO_POINTS, NO_COUNTS)
    assert (r["rc"], len(r["corners"]), r["num_candidates"], r["max_response"]) == (0, 0, 0, 0.0)


@pytest.mark.parametrize("w,h", [(345, 339), (161, 123), (97, 75)])
def test_detection_on_textures(eng, w, h):
    img, lam = image("tex", w, h), lam_of("tex", w, h)
    eng.gft_set_mask(None)
    resident(eng, img)
    for d in (30, 10, 5, 1, 0):
        for mc in (150, 4096):
            want = g.gft(img, max_count=mc, min_distance=d, lam=lam)
            got = eng.gft_detect(NO_POINTS, NO_COUNTS, max_count=mc, min_distance=d)
            print(f"{w} x {h} d {d} max_count {mc}: {want['num_candidates']} candidates, {len(want['corners'])} corners")
            same(got, want)


def test_detection_beyond_one_workgroups_lds(eng):
    img, lam = image("noise", 640, 480), lam_of("noise", 640, 480)
    want = g.gft(img, max_count=500, min_distance=1, lam=lam)
    assert want["num_candidates"] > 20000 and len(want["corners"]) == 500  # 160 KiB of LDS is 20 480 keys: the case cannot go stale
    eng.gft_set_mask(None)
    resident(eng, img)
    same(eng.gft_detect(NO_POINTS, NO_COUNTS, max_count=500, min_distance=1), want)
    # the whole order, not only its head: no distance, the largest budget
    want = g.gft(img, max_count=4096, min_distance=0, lam=lam)
    same(eng.gft_detect(NO_POINTS, NO_COUNTS, max_count=4096, min_distance=0), want)


def test_plateaus_and_ties(eng):
    img, lam = image("tiled", 100, 84), lam_of("tiled", 100, 84)
    inner = lam[8:-8, 8:-8]
    assert len(np.unique(inner)) <= 64 and inner.size > 5000  # hundreds of exactly equal lambda
    eng.gft_set_mask(None)
    resident(eng, img)
    for d, mc in ((3, 4096), (0, 4096), (8, 150), (1, 40)):
        want = g.gft(img, max_count=mc, min_distance=d, lam=lam)
        assert want["num_candidates"] > 100
        same(eng.gft_detect(NO_POINTS, NO_COUNTS, max_count=mc, min_distance=d), want)


def test_masks(eng):
    w, h = 345, 339
    img, lam = image("tex", w, h), lam_of("tex", w, h)
    from lfvio.engine import annulus_mask

    resident(eng, img)
    base = annulus_mask(w, h, 172, 169, 160, 20)
    assert np.array_equal(base, g.annulus_mask(w, h, 172, 169, 160, 20))
    pts, cnt = g.tracked_case(w, h, 0)
    try:
        # the annulus alone
        eng.gft_set_mask(base)
        same(eng.gft_detect(NO_POINTS, NO_COUNTS, max_count=4096, min_distance=5), g.gft(img, base, max_count=4096, min_distance=5, lam=lam))
        # kept points and their discs under the annulus
        want = g.gft(img, base, pts, cnt, max_count=150, min_distance=30, mask_radius=30, lam=lam)
        assert 0 < len(want["kept"]) < len(pts) and 0 < len(want["corners"]) < 150 - len(want["kept"])
        print(f"{len(pts)} points, {len(want['kept'])} kept, {(want['mask'] != 0).mean():.3f} of the mask open, {len(want['corners'])} corners of {want['num_candidates']} candidates")
        same(eng.gft_detect(pts, cnt, max_count=150, min_distance=30, mask_radius=30), want)
        same(eng.gft_detect(pts, cnt, max_count=150, min_distance=10, mask_radius=30), g.gft(img, base, pts, cnt, max_count=150, min_distance=10, mask_radius=30, lam=lam))  # the budget binds
        same(eng.gft_detect(pts, cnt, max_count=4096, min_distance=0, mask_radius=7), g.gft(img, base, pts, cnt, max_count=4096, min_distance=0, mask_radius=7, lam=lam))
        same(eng.gft_detect(pts, cnt, max_count=4096, min_distance=2, mask_radius=0), g.gft(img, base, pts, cnt, max_count=4096, min_distance=2, mask_radius=0, lam=lam))
        # equal counts, a NaN, points outside, the largest N
        rng = np.random.default_rng(11)
        many = np.stack([rng.uniform(-5, w + 5, 4096), rng.uniform(-5, h + 5, 4096)], axis=1).astype(np.float32)
        many[7, 0] = np.nan
        counts = rng.integers(1, 4, 4096).astype(np.int32)
        same(eng.gft_detect(many, counts, max_count=4096, min_distance=3, mask_radius=4), g.gft(img, base, many, counts, max_count=4096, min_distance=3, mask_radius=4, lam=lam))
        # value 128: the point is dropped, the detection is allowed
        grey = np.full((h, w), 255, np.uint8)
        grey[:, :170] = 128
        eng.gft_set_mask(grey)
        want = g.gft(img, grey, pts, cnt, max_count=4096, min_distance=4, mask_radius=12, lam=lam)
        assert (want["corners"][:, 0] < 170).any() and not (pts[want["kept"], 0] < 169.5).any() and (pts[:, 0] < 169).any()
        same(eng.gft_detect(pts, cnt, max_count=4096, min_distance=4, mask_radius=12), want)
        # no budget: max_count <= num_kept
        want = g.gft(img, grey, pts, cnt, max_count=len(want["kept"]), min_distance=4, mask_radius=12, lam=lam)
        assert len(want["kept"]) > 0 and len(want["corners"]) == 0 and want["num_candidates"] == 0
        same(eng.gft_detect(pts, cnt, max_count=len(want["kept"]), min_distance=4, mask_radius=12), want)
        same(eng.gft_detect(pts, cnt, max_count=1, min_distance=4, mask_radius=12), g.gft(img, grey, pts, cnt, max_count=1, min_distance=4, mask_radius=12, lam=lam))
        # an all-zero mask: every point is dropped, no corners
        eng.gft_set_mask(np.zeros((h, w), np.uint8))
        r = eng.gft_detect(pts, cnt)
        assert (r["rc"], len(r["kept"]), len(r["corners"]), r["num_candidates"], r["max_response"]) == (0, 0, 0, 0, 0.0)
        # a mask of another size is refused, and the resident one stays
        assert eng.gft_set_mask(np.zeros((h, w + 1), np.uint8), check=False) == -1
        assert eng.gft_set_mask(np.zeros((8, 8), np.uint8), check=False) == -1
        assert len(eng.gft_detect(pts, cnt)["corners"]) == 0
        # ... also where the image changes under a mask that is set
        small = image("tex", 97, 75)
        resident(eng, small)
        kept, corners = np.full(60, -7, np.int32), np.full((150, 2), -7.0, np.float32)
        r = eng.gft_detect(pts, cnt, kept=kept, corners=corners, check=False)
        assert r["rc"] == -1 and r["num_candidates"] == -1 and np.all(kept == -7) and np.all(corners == -7.0)
        eng.gft_set_mask(None)
        same(eng.gft_detect(NO_POINTS, NO_COUNTS, min_distance=5), g.gft(small, min_distance=5, lam=lam_of("tex", 97, 75)))
    finally:
        eng.gft_set_mask(None)


def test_repeatability_and_isolation(eng):
    c = k.make_case("a", 0)
    w, h = c["img0"].shape[1], c["img0"].shape[0]
    pts, cnt = g.tracked_case(w, h, 0)
    base = g.annulus_mask(w, h, 172, 169, 160, 20)
    eng.gft_set_mask(None)
    eng.klt_reset()
    eng.klt_track(c["img0"], NO_POINTS)
    plain = eng.klt_track(c["img1"], c["pts"])
    try:
        eng.klt_reset()
        eng.klt_track(c["img0"], NO_POINTS)
        eng.gft_set_mask(base)
        runs = [eng.gft_detect(pts, cnt, min_distance=10) for _ in range(5)]
        assert all(same_bits(runs[0], r) for r in runs[1:])
        same(runs[0], g.gft(c["img0"], base, pts, cnt, min_distance=10))
        assert np.array_equal(eng.klt_level(0), c["img0"])
        after = eng.klt_track(c["img1"], c["pts"])  # the resident pyramid was only read
        for f in ("next", "status", "iterations"):
            assert after[f].tobytes() == plain[f].tobytes(), f
        # the base mask survives lfvio_klt_reset (and the calls in between)
        eng.klt_reset()
        r = eng.gft_detect(pts, cnt, check=False)
        assert r["rc"] == -1  # no resident image
        eng.klt_track(c["img0"], NO_POINTS)
        assert same_bits(eng.gft_detect(pts, cnt, min_distance=10), runs[0])
    finally:
        eng.gft_set_mask(None)


REFUSED = [dict(num_points=-1), dict(num_points=4097), dict(max_count=0), dict(max_count=4097), dict(quality_level=0.0), dict(quality_level=-0.01),
           dict(quality_level=1.5), dict(quality_level=float("nan")), dict(min_distance=-1), dict(min_distance=1025), dict(mask_radius=-1), dict(mask_radius=1025)]


def test_argument_errors(eng):
    import ctypes as C

    from lfvio import abi

    img = image("tex", 97, 75)
    pts, cnt = g.tracked_case(97, 75, 0, n=20)
    eng.gft_set_mask(None)
    resident(eng, img)
    want = eng.gft_detect(pts, cnt, min_distance=5, mask_radius=5)
    kept, corners = np.full(4097, -7, np.int32), np.full((4097, 2), -7.0, np.float32)

    def untouched(r):
        return r["rc"] == -1 and r["num_candidates"] == -1 and r["max_response"] == -1.0 and np.all(kept == -7) and np.all(corners == -7.0)

    for over in REFUSED:
        assert untouched(eng.gft_detect(pts, cnt, kept=kept, corners=corners, check=False, **dict(dict(min_distance=5, mask_radius=5), **over))), over
    assert untouched(eng.gft_detect(None, cnt, kept=kept, corners=corners, num_points=20, check=False))
    assert untouched(eng.gft_detect(pts, None, kept=kept, corners=corners, num_points=20, check=False))
    gin, out = abi.GftInC(), abi.GftOutC(-1, -1, -1, -1.0)
    gin.num_points, gin.max_count, gin.quality_level, gin.min_distance, gin.mask_radius = 0, 150, 0.01, 5, 5
    ip, fp = kept.ctypes.data_as(C.POINTER(C.c_int)), corners.ctypes.data_as(C.POINTER(C.c_float))
    assert eng.lib.lfvio_gft_detect(eng.ctx, None, ip, fp, C.byref(out)) == -1
    assert eng.lib.lfvio_gft_detect(eng.ctx, C.byref(gin), ip, None, C.byref(out)) == -1
    assert eng.lib.lfvio_gft_detect(eng.ctx, C.byref(gin), ip, fp, None) == -1
    assert eng.lib.lfvio_gft_detect(None, C.byref(gin), ip, fp, C.byref(out)) == -1
    assert eng.lib.lfvio_gft_response(eng.ctx, None) == -1 and eng.lib.lfvio_gft_set_mask(None, 97, 75, None) == -1
    gin.num_points = 20
    gin.pts, gin.track_cnt = pts.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(C.POINTER(C.c_int))
    assert eng.lib.lfvio_gft_detect(eng.ctx, C.byref(gin), None, fp, C.byref(out)) == -1  # kept is needed where there are points
    assert (out.num_kept, out.num_corners, out.num_candidates, out.max_response) == (-1, -1, -1, -1.0) and np.all(kept == -7) and np.all(corners == -7.0)
    gin.num_points = 0
    assert eng.lib.lfvio_gft_detect(eng.ctx, C.byref(gin), None, fp, C.byref(out)) == 0 and out.num_kept == 0  # ... and not where there are none
    corners[:] = -7.0
    eng.klt_reset()
    assert untouched(eng.gft_detect(pts, cnt, kept=kept, corners=corners, check=False))  # no resident image
    assert eng.klt_level(0, check=False) is None
    resident(eng, img)
    assert same_bits(eng.gft_detect(pts, cnt, min_distance=5, mask_radius=5), want)


def test_beside_an_optimization_in_flight(eng):
    """Between lfvio_batch_optimize_begin and _finish: the optimization's state and prior are the bits of the call without anything in
    between, and the detection is the bits of a call on an idle context."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    win = synth.make_window(0, 300)
    img = image("tex", 345, 339)
    pts, cnt = g.tracked_case(345, 339, 0)
    eng.gft_set_mask(None)
    resident(eng, img)
    alone = eng.gft_detect(pts, cnt, min_distance=10)
    same(alone, g.gft(img, None, pts, cnt, min_distance=10, lam=lam_of("tex", 345, 339)))

    def between(e):
        resident(e, img)
        return e.gft_detect(pts, cnt, min_distance=10)

    def split(e, call):
        e.batch_reserve(1, win.N, win.M)
        e.batch_upload(0, win)
        sol = e.optimize_begin(abi.MARGIN_OLD, win.N)
        res = call(e) if call else None
        return sol, e.optimize_finish(), res

    e0, e1 = Engine(0), Engine(0)
    try:
        sol0, prior0, _ = split(e0, None)
        sol1, prior1, got = split(e1, between)
    finally:
        e0.close()
        e1.close()
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert same_bits(got, alone)
