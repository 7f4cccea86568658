"""CPU tests of the specification of lfvio_gft_detect: tests/gft_ref.py (the numpy restatement of setMask and goodFeaturesToTrack,
DESIGN.md 3l), its fixture tests/golden/gft_cases.npz, and lf-vio_amd/csrc/gft_plan.h — plain C++, compiled here alone with g++ behind
a small ctypes shim, as tests/test_klt_ref.py does for klt_plan.h.

  1  the restatement reproduces its fixture bit for bit, and the fixture is what tests/golden/gen_gft.py writes;
  2  the response against a plain double loop on 16 x 16; the reflection of the PRODUCT maps against the wrong rule (the gradients of
     the reflected image) on an image where they differ, and only in the outermost rows and columns; the tie rule of the order;
  3  truth: a 200 rectangle on 20 has exactly its four corner pixels as candidates and 60 pixels of non-zero response;
  4  setMask: equal counts, distance exactly r and r + 1, base-mask value 128, outside and NaN points, N = 0;
  5  gft_plan.h: every argument limit of LfvioGftIn and of the base mask is refused, the limits themselves are accepted; the sizes of
     the sort network;
  6  include/lfvio.h declares lfvio_gft_detect / _set_mask / _response, abi.HIP_SYMBOLS lists them and the built library exports them."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import gft_ref as g
import klt_ref as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILT = {}


def built():
    """What gen_gft.py writes, computed once and shared."""
    if not BUILT:
        spec = importlib.util.spec_from_file_location("gen_gft", os.path.join(GOLDEN, "gen_gft.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        BUILT.update(gen.build())
    return BUILT


def test_restatement_reproduces_its_fixture():
    b = built()
    path = os.path.join(GOLDEN, "gft_cases.npz")
    assert os.path.getsize(path) < 100 * 1024
    with np.load(path) as z:
        assert sorted(z.files) == sorted(b)
        for key in z.files:
            assert z[key].dtype == b[key].dtype and z[key].shape == b[key].shape and z[key].tobytes() == b[key].tobytes(), key


def test_candidate_counts_of_the_shapes():
    b = built()
    assert [int(b[f"tex_{w}x{h}_d0_m4096_counts"][0]) for w, h in ((345, 339), (161, 123), (97, 75))] == [3119, 540, 187]
    assert int(b["noise_counts"][0]) > 20000 and len(b["noise_corners"]) == 500  # more than one workgroup's LDS holds (20 480 keys)
    for w, h in ((345, 339), (161, 123), (97, 75)):
        n = int(b[f"tex_{w}x{h}_d0_m4096_counts"][0])
        assert len(b[f"tex_{w}x{h}_d0_m4096_corners"]) == n and len(b[f"tex_{w}x{h}_d0_m150_corners"]) == 150  # d = 0 accepts all, up to the budget
        assert np.array_equal(b[f"tex_{w}x{h}_d0_m4096_corners"][:150], b[f"tex_{w}x{h}_d0_m150_corners"])
        for d in (30, 10, 5, 1):
            c = b[f"tex_{w}x{h}_d{d}_m4096_corners"].astype(np.int64)
            d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2) + np.eye(len(c), dtype=np.int64) * d * d
            assert d2.min() >= d * d, (w, h, d)


def loop_response(img):
    h, w = img.shape
    at = lambda x, y: int(img[k.reflect101(y, h), k.reflect101(x, w)])
    dx, dy = np.zeros((h, w), dtype=object), np.zeros((h, w), dtype=object)
    for y in range(h):
        for x in range(w):
            dx[y, x] = (at(x + 1, y - 1) - at(x - 1, y - 1)) + 2 * (at(x + 1, y) - at(x - 1, y)) + (at(x + 1, y + 1) - at(x - 1, y + 1))
            dy[y, x] = (at(x - 1, y + 1) - at(x - 1, y - 1)) + 2 * (at(x, y + 1) - at(x, y - 1)) + (at(x + 1, y + 1) - at(x + 1, y - 1))
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            a = b = c = 0
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    yy, xx = int(k.reflect101(y + j, h)), int(k.reflect101(x + i, w))  # the product maps, reflected
                    a, b, c = a + dx[yy, xx] * dx[yy, xx], b + dx[yy, xx] * dy[yy, xx], c + dy[yy, xx] * dy[yy, xx]
            S, D = a + c, (a - c) * (a - c) + 4 * b * b
            assert math.isqrt(S * S) == S and S * S >= D  # lambda >= 0
            out[y, x] = 0.5 * (float(S) - math.sqrt(float(D)))
    return out


def test_response_against_a_double_loop():
    img = g.noise(16, 16, 3)
    want = loop_response(img)
    got = g.response(img)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert (got >= 0).all() and got.max() > 0
    dx, dy = g.sobel(g.checkerboard(33, 31))
    assert not dx.any() and not dy.any()  # single pixels: both taps of a row see the same grey value
    dx, dy = g.sobel(g.stripes(35, 33, diagonal=True))
    assert np.abs(dx).max() == 1020 and np.abs(dy).max() == 1020  # the bound
    assert g.response(g.stripes(35, 33)).max() == 0.0 and g.response(g.stripes(35, 33, diagonal=True)).max() > 0
    assert np.all(g.response(np.full((20, 24), 77, np.uint8)) == 0.0)


def test_product_maps_are_reflected_not_the_image():
    img = g.textured(97, 75, 0)
    right, wrong = g.response(img), g.response_reflected_image(img)
    differ = right != wrong
    assert differ.any()  # dx changes sign across a vertical edge of the reflected image, and dx dy with it
    assert not differ[1:-1, 1:-1].any()  # ... which only the outermost rows and columns see
    assert differ[0, :].any() and differ[-1, :].any() and differ[:, 0].any() and differ[:, -1].any()


def test_tie_rule_of_the_order():
    lam = np.zeros((7, 9))
    lam[2, 2] = lam[2, 6] = lam[4, 4] = 5.0
    lam[4, 7] = 6.0
    idx, maxv = g.candidates(lam, np.full(lam.shape, 255, np.uint8), 0.01)
    assert maxv == 6.0 and idx.tolist() == [4 * 9 + 7, 4 * 9 + 4, 2 * 9 + 6, 2 * 9 + 2]  # descending lambda, then the larger y * w + x first
    lam[3, 3] = 5.0  # a plateau of two touching pixels: both are candidates
    idx, _ = g.candidates(lam, np.full(lam.shape, 255, np.uint8), 0.01)
    assert idx.tolist() == [4 * 9 + 7, 4 * 9 + 4, 3 * 9 + 3, 2 * 9 + 6, 2 * 9 + 2]
    assert g.pick(idx, 9, 10, 2).tolist() == [[7, 4], [4, 4], [6, 2], [2, 2]]  # (3, 3) is at squared distance 2 < 4 of (4, 4)
    assert g.pick(idx, 9, 2, 0).tolist() == [[7, 4], [4, 4]]
    assert len(g.pick(idx, 9, 10, 0)) == 5


def test_truth_rectangle():
    img = g.truth_image()
    assert img.shape == (48, 64)
    lam = g.response(img)
    assert int((lam != 0).sum()) == 60  # Sobel then the box: a 5 x 5 support; a straight edge alone gives exactly 0
    idx, _ = g.candidates(lam, np.full(img.shape, 255, np.uint8), 0.01)
    assert sorted((int(p) % 64, int(p) // 64) for p in idx) == sorted([(12, 10), (39, 10), (12, 29), (39, 29)])
    r = g.gft(img, min_distance=5)
    assert r["num_candidates"] == 4 and sorted(map(tuple, r["corners"].tolist())) == sorted([(12.0, 10.0), (39.0, 10.0), (12.0, 29.0), (39.0, 29.0)])


def test_set_mask_cases():
    base = np.full((40, 50), 255, np.uint8)
    # equal counts go by index; a higher count goes first
    kept, pix, _ = g.set_mask(base, [[10, 10], [12, 10], [30, 30]], [2, 2, 3], 5)
    assert kept.tolist() == [2, 0] and pix.tolist() == [[30, 30], [10, 10]]
    kept, _, _ = g.set_mask(base, [[12, 10], [10, 10]], [2, 2], 5)
    assert kept.tolist() == [0]
    # distance exactly r is inside the disc, r + 1 is not
    assert g.set_mask(base, [[10, 10], [15, 10]], [2, 1], 5)[0].tolist() == [0]
    assert g.set_mask(base, [[10, 10], [16, 10]], [2, 1], 5)[0].tolist() == [0, 1]
    assert g.set_mask(base, [[10, 10], [13, 14]], [2, 1], 5)[0].tolist() == [0]  # 9 + 16 = 25
    # cvRound: half to even
    assert g.set_mask(base, [[10.5, 11.5]], [1], 0)[1].tolist() == [[10, 12]]
    kept, pix, mask = g.set_mask(base, [[10, 10]], [1], 0)
    assert kept.tolist() == [0] and int((mask == 0).sum()) == 1 and mask[10, 10] == 0  # r = 0: the pixel itself
    # base-mask value 128: the point is dropped, the detection is allowed there
    grey = base.copy()
    grey[:, :25] = 128
    kept, _, mask = g.set_mask(grey, [[10, 10], [40, 10]], [5, 1], 3)
    assert kept.tolist() == [1] and mask[10, 10] == 128 and mask[10, 40] == 0
    img = g.textured(50, 40, 1)
    r = g.gft(img, grey, [[10, 10]], [5], max_count=4096, min_distance=0)
    assert len(r["kept"]) == 0 and (r["corners"][:, 0] < 25).any()
    # outside and NaN points
    pts = np.array([[-0.6, 5], [49.6, 5], [5, 39.6], [np.nan, 5], [5, np.nan], [-0.5, 0], [49.5, 39.5], [np.inf, 3]], np.float32)
    kept, pix, _ = g.set_mask(base, pts, np.arange(8, 0, -1), 2)
    assert kept.tolist() == [5] and pix.tolist() == [[0, 0]]  # -0.5 rounds to 0; 49.5 -> 50 and 39.5 -> 40 are outside
    # N = 0
    kept, pix, mask = g.set_mask(base, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), 30)
    assert len(kept) == 0 and pix.shape == (0, 2) and np.array_equal(mask, base)
    # the discs are Euclidean
    _, _, mask = g.set_mask(base, [[20, 20]], [1], 3)
    assert int((mask == 0).sum()) == 29
    # no budget, an all-zero mask: nothing
    r = g.gft(img, None, [[10, 10], [45, 35]], [1, 1], max_count=2)
    assert len(r["kept"]) == 2 and len(r["corners"]) == 0 and (r["num_candidates"], r["max_response"]) == (0, 0.0)
    r = g.gft(img, np.zeros(img.shape, np.uint8))
    assert len(r["corners"]) == 0 and (r["num_candidates"], r["max_response"]) == (0, 0.0)


def test_masked_case():
    b = built()
    assert (len(b["masked_pts"]), len(b["masked_kept"]), len(b["masked_corners"]), int(b["masked_counts"][0])) == (60, 21, 46, 964)
    from lfvio.engine import annulus_mask

    assert np.array_equal(annulus_mask(345, 339, 172, 169, 160, 20), g.annulus_mask(345, 339, 172, 169, 160, 20))
    m = annulus_mask(64, 48, 30, 20, 10, 3)
    assert m[20, 40] == 255 and m[20, 41] == 0 and m[20, 33] == 0 and m[20, 34] == 255 and set(np.unique(m)) == {0, 255}


# ---- gft_plan.h behind a ctypes shim
SRC = r'''
#include "gft_plan.h"
static float POINT[2];
static int COUNT;
extern "C" const char *gp_check(int n, int null_pts, int null_cnt, int max_count, double quality, int min_distance, int mask_radius) {
  LfvioGftIn in;
  in.num_points = n, in.pts = null_pts ? nullptr : POINT, in.track_cnt = null_cnt ? nullptr : &COUNT;
  in.max_count = max_count, in.quality_level = quality, in.min_distance = min_distance, in.mask_radius = mask_radius;
  return gft_check(&in);
}
extern "C" const char *gp_mask_check(int w, int h, int iw, int ih) { return gft_mask_check(w, h, iw, ih); }
extern "C" long long gp_capacity(int w, int h) { return (long long)gft_capacity(w, h); }
extern "C" int gp_launches(long long capacity) { return gft_sort_launches((size_t)capacity); }
extern "C" int gp_consts(int *out) {
  const int v[] = {LFVIO_GFT_MAX_CORNERS, GFT_MAX_DIST, GFT_CHUNK, (int)sizeof(LfvioGftIn), (int)sizeof(LfvioGftOut)};
  for (unsigned k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
  return (int)(sizeof v / sizeof v[0]);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="gft_plan_")
    src, so = os.path.join(d, "gp.cpp"), os.path.join(d, "libgp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.gp_check.restype = C.c_char_p
    so.gp_check.argtypes = [C.c_int] * 4 + [C.c_double] + [C.c_int] * 2
    so.gp_mask_check.restype = C.c_char_p
    so.gp_mask_check.argtypes = [C.c_int] * 4
    so.gp_capacity.restype = C.c_longlong
    so.gp_capacity.argtypes = [C.c_int] * 2
    so.gp_launches.argtypes = [C.c_longlong]
    return so


GOOD = dict(n=60, null_pts=0, null_cnt=0, max_count=150, quality=0.01, min_distance=30, mask_radius=30)
ORDER = ("n", "null_pts", "null_cnt", "max_count", "quality", "min_distance", "mask_radius")
REFUSED = [dict(n=-1), dict(n=4097), dict(null_pts=1), dict(null_cnt=1), dict(max_count=0), dict(max_count=4097), dict(quality=0.0), dict(quality=-0.01),
           dict(quality=1.0000001), dict(quality=float("nan")), dict(min_distance=-1), dict(min_distance=1025), dict(mask_radius=-1), dict(mask_radius=1025)]
ACCEPTED = [dict(), dict(n=0), dict(n=0, null_pts=1, null_cnt=1), dict(n=4096), dict(max_count=1), dict(max_count=4096), dict(quality=1e-300), dict(quality=1.0),
            dict(min_distance=0), dict(min_distance=1024), dict(mask_radius=0), dict(mask_radius=1024)]


def test_argument_limits(lib):
    check = lambda over: lib.gp_check(*[dict(GOOD, **over)[f] for f in ORDER])
    for over in ACCEPTED:
        assert check(over) is None, over
    for over in REFUSED:
        why = check(over)
        assert why is not None and why.startswith(b"lfvio_gft_detect: "), over
    for w, h, iw, ih in ((16, 16, 0, 0), (8192, 8192, 0, 0), (345, 339, 345, 339)):
        assert lib.gp_mask_check(w, h, iw, ih) is None
    for w, h, iw, ih in ((15, 16, 0, 0), (16, 15, 0, 0), (8193, 16, 0, 0), (16, 8193, 0, 0), (345, 339, 345, 338), (345, 339, 344, 339), (339, 345, 345, 339)):
        assert lib.gp_mask_check(w, h, iw, ih).startswith(b"lfvio_gft_set_mask: ")


def test_plan_header_constants_and_sizes(lib):
    from lfvio import abi

    out = (C.c_int * 8)()
    assert lib.gp_consts(out) == 5
    assert out[:5] == [abi.GFT_MAX_CORNERS, g.MAX_RADIUS, 4096, C.sizeof(abi.GftInC), C.sizeof(abi.GftOutC)]
    assert (g.MAX_CORNERS, g.MAX_POINTS) == (abi.GFT_MAX_CORNERS, abi.KLT_MAX_POINTS)
    # a plateau makes every interior pixel a candidate: the capacity covers every pixel, as a power of two of at least one chunk
    for w, h, cap in ((16, 16, 4096), (64, 64, 4096), (65, 64, 8192), (345, 339, 131072), (640, 480, 524288), (1280, 960, 2097152), (8192, 8192, 1 << 26)):
        assert lib.gp_capacity(w, h) == cap
    assert [lib.gp_launches(c) for c in (4096, 8192, 16384, 2097152)] == [1, 3, 6, 55]


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi
    from lfvio.engine import Engine

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("lfvio_gft_detect", "lfvio_gft_set_mask", "lfvio_gft_response"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+LFVIO_GFT_MAX_CORNERS\s+4096\b", src)
    for name in ("gft_set_mask", "gft_detect", "gft_response"):
        assert callable(getattr(Engine, name))
