"""lfvio_clahe_apply / lfvio_clahe_set (kernels_clahe.h) against the numpy restatement tests/clahe_ref.py, which is the specification
(tests/test_clahe_ref.py holds it to its fixture).  Everything is compared bit for bit: no tolerance, nothing excluded.  The cases are
clahe_ref.CASES: seeded images at the smallest shapes that reach each path.

  1  clahe_apply equals the restatement, image and LUTs, on every case;
  2  with clahe_set on: level 0 after klt_track is the restatement of the image, the higher levels are klt_ref's pyramid of it, a
     tracked pair gives the bytes of the same pair equalized on the host and tracked with the setting off, gft_detect equals gft_ref
     on the equalized image;
  3  a fresh context does not equalize, clahe_set(None) restores that, the setting survives klt_reset and a change of image size,
     clahe_apply leaves the setting and the resident image alone;
  4  argument errors leave the outputs (0x5A-filled) and the setting untouched;
  5  repeatability, also with two image sizes alternating;
  6  beside an optimization in flight."""
import ctypes as C
import functools

import numpy as np
import pytest

import clahe_ref as c
import gft_ref as g
import klt_ref as k

pytestmark = pytest.mark.gpu
NO_POINTS = np.zeros((0, 2), np.float32)
NO_COUNTS = np.zeros(0, np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, clip_limit, tiles, the restatement's image, its LUTs), computed once and read-only."""
    cl, tiles = c.CASES[name][4:]
    img = c.case_image(name)
    out, lut = c.clahe(img, cl, tiles)
    for a in (img, out, lut):
        a.setflags(write=False)
    return img, cl, tiles, out, lut


def resident(eng, img):
    """img made resident without tracking (N = 0)."""
    assert eng.klt_track(img, NO_POINTS, want_iterations=False)["rc"] == 0


@pytest.mark.parametrize("name", sorted(c.CASES))
def test_apply_equals_the_restatement(eng, name):
    img, cl, tiles, want, want_lut = case(name)
    got, lut = eng.clahe_apply(img, cl, tiles, want_lut=True)
    assert got.dtype == np.uint8 and got.shape == want.shape and lut.shape == want_lut.shape
    print(f"{name}: {int((lut != want_lut).sum())} of {lut.size} LUT entries and {int((got != want).sum())} of {got.size} pixels differ")
    assert np.array_equal(lut, want_lut), np.argwhere(lut != want_lut)[:8]
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(eng.clahe_apply(img, cl, tiles), want)  # without the LUTs


def test_setting_on_level_zero_and_the_pyramid(eng):
    try:
        for name in ("texture_345x339", "neither_97x75", "divides_64"):
            img, cl, tiles, want, _ = case(name)
            eng.clahe_set(cl, tiles)
            eng.klt_reset()
            r = eng.klt_track(img, NO_POINTS, win_size=5, max_level=3)
            levels = k.pyramid(want, 5, 3)
            assert r["levels_used"] == len(levels) - 1 >= 2
            for lv, ref in enumerate(levels):
                assert np.array_equal(eng.klt_level(lv), ref), (name, lv)
    finally:
        eng.clahe_set(None)


def test_setting_on_tracking_and_detection(eng):
    """161 x 123, 40 points: the pair equalized on the device and the pair equalized by the restatement and tracked with the setting
    off give the same bytes; gft_detect right after sees the equalized image."""
    w, h, n = 161, 123, 40
    f = k.texture(0)
    fwd, inv = k.warp(w, h, (2.3, -1.6))
    img0, img1 = k.render(f, w, h), k.render(f, w, h, inv)
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(20, w - 21, n), rng.uniform(20, h - 21, n)], axis=1).astype(np.float32)
    eq0, eq1 = c.clahe(img0)[0], c.clahe(img1)[0]
    assert (eq0 != img0).any()
    kw = dict(win_size=21, max_level=3)
    eng.clahe_set(None)
    eng.gft_set_mask(None)
    eng.klt_reset()
    eng.klt_track(eq0, NO_POINTS, **kw)
    want = eng.klt_track(eq1, pts, **kw)
    assert want["num_tracked"] > n // 2
    try:
        eng.clahe_set(3.0, (8, 8))
        eng.klt_reset()
        eng.klt_track(img0, NO_POINTS, **kw)
        got = eng.klt_track(img1, pts, **kw)
        for fld in ("next", "status", "iterations"):
            assert got[fld].tobytes() == want[fld].tobytes(), fld
        assert (got["levels_used"], got["num_tracked"]) == (want["levels_used"], want["num_tracked"])
        assert np.array_equal(eng.klt_level(0), eq1)
        cnt = np.ones(n, np.int32)
        det = eng.gft_detect(got["next"], cnt, min_distance=10, mask_radius=10)
        ref = g.gft(eq1, None, got["next"], cnt, min_distance=10, mask_radius=10)
        assert len(ref["corners"]) > 0
        assert np.array_equal(det["kept"], ref["kept"]) and det["corners"].tobytes() == ref["corners"].tobytes()
        assert det["num_candidates"] == ref["num_candidates"] and det["max_response"] == ref["max_response"]
        assert eng.gft_response().tobytes() == g.response(eq1).tobytes()
    finally:
        eng.clahe_set(None)
    # ... and with the setting off again the raw pair tracks as it did before this feature: not the equalized result
    eng.klt_reset()
    eng.klt_track(img0, NO_POINTS, **kw)
    raw = eng.klt_track(img1, pts, **kw)
    assert np.array_equal(eng.klt_level(0), img1) and raw["next"].tobytes() != want["next"].tobytes()


def test_default_and_persistence():
    from lfvio.engine import Engine

    a, _, _, eq_a, _ = case("neither_97x75")
    b, _, _, eq_b, _ = case("track_161x123")
    e = Engine(0)
    try:
        resident(e, a)  # a fresh context does not equalize
        assert np.array_equal(e.klt_level(0), a)
        e.clahe_set(3.0, (8, 8))
        resident(e, a)
        assert np.array_equal(e.klt_level(0), eq_a)
        e.klt_reset()  # the setting survives lfvio_klt_reset
        assert e.klt_level(0, check=False) is None
        resident(e, a)
        assert np.array_equal(e.klt_level(0), eq_a)
        resident(e, b)  # ... and a change of image size
        assert np.array_equal(e.klt_level(0), eq_b)
        # clahe_apply with another configuration: neither the setting nor the resident image moves
        other = e.clahe_apply(a, 0.0, (3, 5))
        assert np.array_equal(other, c.clahe(a, 0.0, (3, 5))[0]) and (other != eq_a).any()
        assert np.array_equal(e.klt_level(0), eq_b)
        resident(e, a)
        assert np.array_equal(e.klt_level(0), eq_a)
        e.clahe_set(2.0, (3, 5))  # another setting replaces the first
        resident(e, a)
        assert np.array_equal(e.klt_level(0), c.clahe(a, 2.0, (3, 5))[0])
        e.clahe_set(None)  # off again
        resident(e, a)
        assert np.array_equal(e.klt_level(0), a)
        assert np.array_equal(e.clahe_apply(a), eq_a)  # apply does not need the setting
        resident(e, b)
        assert np.array_equal(e.klt_level(0), b)
    finally:
        e.close()


REFUSED = [dict(clip_limit=-0.5), dict(clip_limit=1024.5), dict(clip_limit=float("nan")), dict(clip_limit=float("inf")), dict(tiles=(0, 8)), dict(tiles=(8, 0)),
           dict(tiles=(17, 8)), dict(tiles=(8, 17)), dict(tiles=(-1, 8)), dict(size=(15, 75)), dict(size=(97, 15)), dict(size=(8193, 75)), dict(size=(97, 8193)),
           dict(size=(0, 0)), dict(size=(-97, 75))]


def test_argument_errors(eng):
    from lfvio import abi

    img, cl, tiles, want, want_lut = case("neither_97x75")
    up = C.POINTER(C.c_ubyte)
    out, lut = np.full((8192 + 64,), 0x5A, np.uint8), np.full((16, 16, 256), 0x5A, np.uint8)

    def untouched():
        return np.all(out == 0x5A) and np.all(lut == 0x5A)

    try:
        eng.clahe_set(cl, tiles)
        resident(eng, img)
        for over in REFUSED:
            args = dict(dict(clip_limit=cl, tiles=tiles), **over)
            rc, _, _ = eng.clahe_apply(img, out=out, lut=lut, check=False, **args)
            assert rc == -1 and untouched(), over
            if "size" not in over:
                assert eng.clahe_set(args["clip_limit"], args["tiles"], check=False) == -1, over
        rc, _, _ = eng.clahe_apply(None, cl, tiles, out=out, lut=lut, size=(97, 75), check=False)
        assert rc == -1 and untouched()
        cin = abi.ClaheInC(cl, tiles[0], tiles[1])
        px, po, pl = img.ctypes.data_as(up), out.ctypes.data_as(up), lut.ctypes.data_as(up)
        assert eng.lib.lfvio_clahe_apply(eng.ctx, None, 97, 75, px, po, pl) == -1
        assert eng.lib.lfvio_clahe_apply(eng.ctx, C.byref(cin), 97, 75, px, None, pl) == -1
        assert eng.lib.lfvio_clahe_apply(None, C.byref(cin), 97, 75, px, po, pl) == -1
        assert eng.lib.lfvio_clahe_set(None, C.byref(cin)) == -1 and eng.lib.lfvio_clahe_set(None, None) == -1
        assert untouched()
        # the resident image and the setting are what they were
        assert np.array_equal(eng.klt_level(0), want)
        resident(eng, img)
        assert np.array_equal(eng.klt_level(0), want)
        # a null lut is not an error
        big = np.full((75, 97), 0x5A, np.uint8)
        assert eng.lib.lfvio_clahe_apply(eng.ctx, C.byref(cin), 97, 75, px, big.ctypes.data_as(up), None) == 0 and np.array_equal(big, want)
        # the limits themselves are accepted
        for cl2, t2 in ((0.0, (1, 1)), (1024.0, (16, 16)), (1024.0, (1, 16))):
            got, l2 = eng.clahe_apply(img, cl2, t2, want_lut=True)
            ref = c.clahe(img, cl2, t2)
            assert np.array_equal(got, ref[0]) and np.array_equal(l2, ref[1]), (cl2, t2)
    finally:
        eng.clahe_set(None)


def test_repeatability(eng):
    a, cl, tiles, want_a, lut_a = case("texture_345x339")
    b, _, _, want_b, lut_b = case("neither_97x75")
    for _ in range(3):  # the grow-only buffers, and the int table left zero by the call before
        for img, want, want_lut in ((a, want_a, lut_a), (b, want_b, lut_b), (b, want_b, lut_b)):
            got, lut = eng.clahe_apply(img, cl, tiles, want_lut=True)
            assert np.array_equal(got, want) and np.array_equal(lut, want_lut)
    try:
        eng.clahe_set(cl, tiles)
        for _ in range(2):
            for img, want in ((a, want_a), (b, want_b)):
                resident(eng, img)
                assert np.array_equal(eng.klt_level(0), want)
                assert np.array_equal(eng.clahe_apply(b, 0.0, (16, 16)), c.clahe(b, 0.0, (16, 16))[0])  # another tile count in between
    finally:
        eng.clahe_set(None)


def test_beside_an_optimization_in_flight():
    """Between lfvio_batch_optimize_begin and _finish: the optimization's state and prior are the bits of the call without anything in
    between, and the equalized image is the restatement's."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    win = synth.make_window(0, 300)
    img, cl, tiles, want, want_lut = case("texture_345x339")

    def between(e):
        return e.clahe_apply(img, cl, tiles, want_lut=True)

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
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want_lut)
