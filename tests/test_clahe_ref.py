"""CPU tests of the specification of lfvio_clahe_set / lfvio_clahe_apply: tests/clahe_ref.py (the numpy restatement of OpenCV's 8-bit
CLAHE), its fixture tests/golden/clahe_cases.npz, and lf-vio_amd/csrc/clahe_plan.h — plain C++, compiled here alone with
g++ behind a small ctypes shim, as tests/test_gft_ref.py does for gft_plan.h.  Everything is compared bit for bit.

  1  the restatement reproduces its fixture, and the fixture is what tests/golden/gen_clahe.py writes;
  2  a literal scalar double-loop transcription of the algorithm equals the vectorised restatement on 40 x 56 and 97 x 75, LUTs and image;
  3  constant images: the LUT entry and the output value worked out by hand from area, clip, batch and residual;
  4  the fused-multiply-add variant of the interpolation differs from the specification on at least one pixel of every case of
     clahe_ref.CASES whose weights are not dyadic (and on none whose weights are), so the device comparison sees contraction;
  5  on 96 x 75 with 8 x 8 tiles the "pad only the side that does not divide" variant differs: the quirk is pinned;
  6  clahe_plan.h: tw, th, clip and the bit patterns of lut_scale, inv_tw, inv_th equal the restatement's over a sweep; the argument
     limits are accepted and refused as stated;
  7  include/lfvio.h declares lfvio_clahe_set / _apply, abi.HIP_SYMBOLS lists them and the built library exports them;
  8  what the cases of clahe_ref.CASES are said to reach, they reach."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import clahe_ref as c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILT = {}


def built():
    """What gen_clahe.py writes, computed once and shared."""
    if not BUILT:
        spec = importlib.util.spec_from_file_location("gen_clahe", os.path.join(GOLDEN, "gen_clahe.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        BUILT.update(gen.build())
    return BUILT


def test_restatement_reproduces_its_fixture():
    b = built()
    path = os.path.join(GOLDEN, "clahe_cases.npz")
    assert os.path.getsize(path) < 100 * 1024
    with np.load(path) as z:
        assert sorted(z.files) == sorted(b)
        for key in z.files:
            assert z[key].dtype == np.uint8 and z[key].shape == b[key].shape and z[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("w,h,clip_limit,tiles,kind", [(40, 56, 3.0, (8, 8), "tex"), (97, 75, 3.0, (8, 8), "tex"), (97, 75, 40.0, (3, 5), "noise"),
                                                       (40, 56, 0.0, (4, 7), "noise"), (16, 31, 2.0, (16, 16), "noise")])
def test_literal_loops_equal_the_restatement(w, h, clip_limit, tiles, kind):
    img = c.textured(w, h, 5) if kind == "tex" else c.noise(w, h, 5)
    out, lut = c.clahe(img, clip_limit, tiles)
    loop_out, loop_lut = c.clahe_loops(img, clip_limit, tiles)
    assert np.array_equal(lut, loop_lut) and np.array_equal(out, loop_out)
    assert out.shape == img.shape and lut.shape == (tiles[1], tiles[0], 256)


def test_constant_images_by_hand():
    # 64 x 64 of value 99, 8 x 8 tiles, clip_limit 3: area 64, clip = max((int)(3 * 64 / 256), 1) = max(0, 1) = 1.  The one bin of 64
    # is cut to 1, clipped = 63: batch 0, residual 63, step 256 / 63 = 4, so the bins 0, 4, .., 248 take one each.  Up to bin 99 that
    # is the 25 bins 0 .. 96 and bin 99 itself: 26.  26 * 255 / 64 = 103.59 -> 104, in every tile, so every pixel is 104.
    p = c.plan(64, 64, 3.0, (8, 8))
    assert (p["area"], p["clip"]) == (64, 1)
    out, lut = c.clahe(np.full((64, 64), 99, np.uint8), 3.0, (8, 8))
    assert np.all(lut[:, :, 99] == 104) and np.all(out == 104)
    assert np.all(lut[:, :, 0] == 4) and np.all(lut[:, :, 255] == 255)  # 1 * 255 / 64 = 3.98; all 64 counts: 255
    # 128 x 128 of value 99, 2 x 2 tiles: area 4096, clip (int)(3 * 4096 / 256) = 48; clipped = 4096 - 48 = 4048: batch 15, residual
    # 4048 - 3840 = 208, step 1: the bins 0 .. 207 hold 16, the others 15, bin 99 holds 48 + 15 + 1 = 64.  Up to bin 99: 99 * 16 + 64 =
    # 1648; 1648 * 255 / 4096 = 102.6 -> 103.
    p = c.plan(128, 128, 3.0, (2, 2))
    assert (p["area"], p["clip"]) == (4096, 48)
    out, lut = c.clahe(np.full((128, 128), 99, np.uint8), 3.0, (2, 2))
    assert np.all(lut[:, :, 99] == 103) and np.all(out == 103)
    assert np.all(lut[:, :, 98] == 99)  # 99 * 16 = 1584; 1584 * 255 / 4096 = 98.6
    # no clipping: the LUT is the step 0 -> 255 at the value, the image becomes 255
    out, lut = c.clahe(np.full((64, 64), 99, np.uint8), 0.0, (8, 8))
    assert np.all(lut[:, :, :99] == 0) and np.all(lut[:, :, 99:] == 255) and np.all(out == 255)


@pytest.mark.parametrize("name", sorted(c.CASES))
def test_fusing_changes_the_bytes_where_weights_are_not_dyadic(name):
    cl, tiles = c.CASES[name][4:]
    img = c.case_image(name)
    lut = c.luts(img, cl, tiles)
    n = int((c.interpolate(img, lut, tiles) != c.interpolate(img, lut, tiles, fused=True)).sum())
    print(f"{name}: {n} of {img.size} pixels differ when each product-sum pair is fused")
    if c.dyadic(name):
        assert n == 0
    else:
        assert n >= 1


def test_a_side_that_divides_is_padded_too():
    img = c.case_image("one_side_96x75")
    assert c.extent(96, 75, (8, 8)) == (104, 80) and c.extent(96, 75, (8, 8), pad_both=False) == (96, 80)
    assert c.extent(96, 80, (8, 8)) == (96, 80) and c.extent(97, 75, (3, 5)) == (99, 80)
    spec, variant = c.clahe(img, 3.0, (8, 8)), c.clahe(img, 3.0, (8, 8), pad_both=False)
    assert (spec[0] != variant[0]).any() and (spec[1] != variant[1]).any()


def test_cases_reach_what_they_are_said_to():
    p = c.plan(16, 16, 3.0, (8, 8))
    assert (p["tw"], p["th"], p["area"], p["clip"]) == (2, 2, 4, 1)
    p = c.plan(16, 31, 3.0, (16, 16))
    assert (p["ext_w"], p["ext_h"]) == (32, 32)
    ext = c.extended(c.case_image("repeated_16x31"), (16, 16))
    assert np.array_equal(ext[:31, 31], c.case_image("repeated_16x31")[:, 1])  # column 31 -> -1 -> 1: reflected twice
    # clip_limit 40: the clip is above every bin of every tile
    img = c.case_image("clip40_nothing_clipped")
    p = c.plan(97, 75, 40.0, (8, 8))
    assert p["clip"] == 20 and c.histograms(img, (8, 8)).max() < 20
    assert np.array_equal(c.luts(img, 40.0, (8, 8)), c.luts(img, 0.0, (8, 8)))
    # the residuals 1, 127, 129, 255, without and with a batch
    for name, batch in (("residuals", 0), ("residuals_batch", 1)):
        hist = c.histograms(c.case_image(name), (2, 2))
        assert c.plan(64, 64, 3.0, (2, 2))["clip"] == c.RESIDUAL_CLIP
        clipped = np.maximum(hist - c.RESIDUAL_CLIP, 0).sum(axis=-1)
        assert np.array_equal(clipped.ravel(), [256 * batch + r for r in c.RESIDUALS])
        assert np.array_equal(c.redistribute(hist, c.RESIDUAL_CLIP)[1].ravel(), c.RESIDUALS)
    # the two-valued image: two bins per tile at most
    assert (c.histograms(c.case_image("two_valued_97x75"), (8, 8)) > 0).sum(axis=-1).max() <= 2
    # the kinds of size the device code distinguishes: widths that are and are not a multiple of 4, more than one 256-column block
    widths = {c.CASES[n][1] for n in c.CASES}
    assert {w % 4 == 0 for w in widths} == {True, False} and max(widths) > 512


# ---- clahe_plan.h behind a ctypes shim
SRC = r'''
#include "clahe_plan.h"
extern "C" const char *cp_check(double clip_limit, int tx, int ty) {
  LfvioClaheIn in;
  in.clip_limit = clip_limit, in.tiles_x = tx, in.tiles_y = ty;
  return clahe_check(&in);
}
extern "C" const char *cp_size_check(int w, int h) { return clahe_size_check(w, h); }
extern "C" void cp_plan(int w, int h, double clip_limit, int tx, int ty, int *out, float *f) {
  LfvioClaheIn in;
  in.clip_limit = clip_limit, in.tiles_x = tx, in.tiles_y = ty;
  const ClahePlan p = clahe_plan(w, h, in);
  out[0] = p.ext_w, out[1] = p.ext_h, out[2] = p.tw, out[3] = p.th, out[4] = p.area, out[5] = p.clip;
  f[0] = p.lut_scale, f[1] = p.inv_tw, f[2] = p.inv_th;
}
extern "C" int cp_consts(int *out) {
  const int v[] = {LFVIO_CLAHE_MAX_TILES, (int)CLAHE_MAX_CLIP, (int)sizeof(LfvioClaheIn), (int)sizeof(LfvioKltIn)};
  for (unsigned k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
  return (int)(sizeof v / sizeof v[0]);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="clahe_plan_")
    src, so = os.path.join(d, "cp.cpp"), os.path.join(d, "libcp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.cp_check.restype = C.c_char_p
    so.cp_check.argtypes = [C.c_double, C.c_int, C.c_int]
    so.cp_size_check.restype = C.c_char_p
    so.cp_size_check.argtypes = [C.c_int, C.c_int]
    so.cp_plan.restype = None
    so.cp_plan.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return so


def test_plan_equals_the_restatement(lib):
    sizes = [(16, 16), (16, 31), (64, 64), (97, 75), (96, 75), (161, 123), (345, 339), (640, 480), (1280, 960), (752, 480), (8192, 8192), (8191, 17)]
    tiles = [(8, 8), (1, 1), (3, 5), (16, 16), (7, 16), (16, 1)]
    clips = [0.0, 3.0, 40.0, 0.5, 2.999999, 1e-9, 1024.0]
    ints, floats = (C.c_int * 6)(), (C.c_float * 3)()
    n = 0
    for w, h in sizes:
        for t in tiles:
            for cl in clips:
                lib.cp_plan(w, h, cl, t[0], t[1], ints, floats)
                p = c.plan(w, h, cl, t)
                assert list(ints) == [p[f] for f in ("ext_w", "ext_h", "tw", "th", "area", "clip")], (w, h, t, cl)
                got = np.array(list(floats), np.float32).view(np.uint32)
                want = np.array([p["lut_scale"], p["inv_tw"], p["inv_th"]], np.float32).view(np.uint32)
                assert np.array_equal(got, want), (w, h, t, cl)
                n += 1
    assert n == len(sizes) * len(tiles) * len(clips)
    lib.cp_plan(8192, 8192, 1024.0, 1, 1, ints, floats)
    assert ints[5] == 4 * 8192 * 8192  # the largest clip fits an int


def test_argument_limits(lib):
    from lfvio import abi

    for cl, tx, ty in ((3.0, 8, 8), (0.0, 1, 1), (1024.0, 16, 16), (1e-300, 1, 16), (-0.0, 16, 1)):
        assert lib.cp_check(cl, tx, ty) is None, (cl, tx, ty)
    for cl, tx, ty in ((-1e-9, 8, 8), (1024.0000001, 8, 8), (float("nan"), 8, 8), (float("inf"), 8, 8), (3.0, 0, 8), (3.0, 8, 0), (3.0, 17, 8), (3.0, 8, 17),
                       (3.0, -1, 8), (3.0, 8, -8)):
        why = lib.cp_check(cl, tx, ty)
        assert why is not None and why.startswith(b"lfvio_clahe: "), (cl, tx, ty)
    for w, h in ((16, 16), (8192, 8192), (16, 8192), (1280, 960)):
        assert lib.cp_size_check(w, h) is None
    for w, h in ((15, 16), (16, 15), (8193, 16), (16, 8193), (0, 0), (-16, 64)):
        assert lib.cp_size_check(w, h).startswith(b"lfvio_clahe_apply: ")
    out = (C.c_int * 8)()
    assert lib.cp_consts(out) == 4
    assert out[:3] == [abi.CLAHE_MAX_TILES, int(c.MAX_CLIP), C.sizeof(abi.ClaheInC)] and out[3] == C.sizeof(abi.KltInC)
    assert (c.MAX_TILES, c.MIN_SIDE, c.MAX_SIDE) == (abi.CLAHE_MAX_TILES, 16, 8192)


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi
    from lfvio.engine import Engine

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("lfvio_clahe_set", "lfvio_clahe_apply"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+LFVIO_CLAHE_MAX_TILES\s+16\b", src)
    for name in ("clahe_set", "clahe_apply"):
        assert callable(getattr(Engine, name))
