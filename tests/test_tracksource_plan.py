"""CPU tests of lf-vio_amd/csrc/tracksource_plan.h — the plain C++ behind lfvio_track_source_set — compiled alone with g++
-ffp-contract=off -Wall -Werror behind a ctypes shim and held to tests/tracksource_ref.py.

  1  the per-call check on every refusal of include/lfvio.h, each beside a neighbour that is accepted: no resident map, a resident map
     of another width or height, a source side of 15 or 8193, an encoding outside the table, a step below src_width * bytes per pixel
     (judged beside the SOURCE's width, not the tracked image's) and above 65536, with the format setting off and on; the setting off
     accepts everything.  The order is the header's: the map before the format.  The plan's bytes are src_height * step.
  2  the host copy of one lane of k_remap_gray, run for every lane of the launch, equals image_ref.to_gray of project_ref.remap bit for
     bit for all six encodings (and the seventh, rgba8) at 131 x 67 — 8777 pixels, 1 mod 4: the last lane takes the tail of one — and at
     128 x 64, through an equirectangular map and a perspective one, with a padded odd step and without; every map has entries inside
     and outside the source, so both the gather and the select run; the output array has exactly width * height bytes and the guard
     bytes behind it stay, so lanes past the last pixel write nothing.
  3  the launch geometry: whole workgroups of 256 lanes of 4 pixels, as k_remap_apply's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import image_ref as ir
import project_ref as pr
import tracksource_ref as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstring>
#include <vector>

#include "tracksource_plan.h"
static TrackSourceState state(int on, int sw, int sh) {
  TrackSourceState s;
  s.on = on != 0, s.sw = sw, s.sh = sh;
  return s;
}
extern "C" const char *ts_call_check(int on, int sw, int sh, int valid, int rw, int rh, int null_fmt, int encoding, int step, int W, int H) {
  RemapResident r;
  r.valid = valid != 0, r.width = rw, r.height = rh;
  const LfvioImageFormat f = {encoding, step};
  return tracksource_call_check(state(on, sw, sh), r, null_fmt ? nullptr : &f, W, H);
}
// out: bytes, sw, sh, step, bpp, code
extern "C" void ts_plan(int sw, int sh, int null_fmt, int encoding, int step, long long *out) {
  const LfvioImageFormat f = {encoding, step};
  const TrackSourcePlan p = tracksource_plan(state(1, sw, sh), null_fmt ? nullptr : &f);
  out[0] = (long long)p.bytes, out[1] = p.g.sw, out[2] = p.g.sh, out[3] = p.g.step, out[4] = p.g.bpp, out[5] = p.code;
}
// every lane of the launch; the integer map from the float maps by remap_offset.  Returns the number of lanes; counts: inside, outside
extern "C" long long ts_level0(int encoding, int step, int sw, int sh, long long pixels, const float *mx, const float *my, const unsigned char *src,
                               unsigned char *level0, long long *counts) {
  const LfvioImageFormat f = {encoding, step};
  const RemapGeom g = remap_geom(f, sw, sh);
  std::vector<int> imap((size_t)pixels);
  counts[0] = counts[1] = 0;
  for (size_t p = 0; p < (size_t)pixels; p++) imap[p] = remap_offset(mx[p], my[p], g), counts[imap[p] < 0]++;
  const size_t lanes = tracksource_lanes((size_t)pixels);
  for (size_t lane = 0; lane < lanes; lane++) tracksource_lane(encoding, imap.data(), src, level0, (size_t)pixels, lane);
  return (long long)lanes;
}
extern "C" void ts_geometry(long long pixels, long long *out) { out[0] = tracksource_blocks((size_t)pixels), out[1] = (long long)tracksource_lanes((size_t)pixels); }
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="tracksource_plan_")
    src, so = os.path.join(d, "ts.cpp"), os.path.join(d, "libts.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    i, ll, fp, up, lp = C.c_int, C.c_longlong, C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)
    so.ts_call_check.restype, so.ts_call_check.argtypes = C.c_char_p, [i] * 11
    so.ts_plan.restype, so.ts_plan.argtypes = None, [i] * 5 + [lp]
    so.ts_level0.restype, so.ts_level0.argtypes = ll, [i, i, i, i, ll, fp, fp, up, up, lp]
    so.ts_geometry.restype, so.ts_geometry.argtypes = None, [ll, lp]
    return so


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def says(lib, source=(161, 123), resident=(131, 67), fmt=(2, 0), size=(131, 67)):
    """The header's verdict (None: accepted), after agreeing with the numpy text on whether the call is refused."""
    on, (sw, sh) = source is not None, source or (0, 0)
    valid, (rw, rh) = resident is not None, resident or (0, 0)
    enc, step = fmt or (0, 0)
    got = lib.ts_call_check(on, sw, sh, valid, rw, rh, fmt is None, enc, step, size[0], size[1])
    want = ts.call_check(source, resident, fmt, size[0], size[1])
    assert (got is None) == (want is None), (source, resident, fmt, size, got, want)
    return got


# ---- 1
def test_call_check(lib):
    assert says(lib) is None and says(lib, fmt=None) is None and says(lib, fmt=(2, 487)) is None
    # off: nothing is judged
    assert says(lib, source=None, resident=None, fmt=(9, -1), size=(1, 1)) is None
    assert b"no resident map" in says(lib, resident=None)
    for other in ((130, 67), (131, 66), (67, 131), (161, 123)):
        assert b"another size" in says(lib, resident=other)
    assert says(lib, resident=(161, 123), size=(161, 123)) is None
    # the map before the format
    assert b"no resident map" in says(lib, resident=None, fmt=(1, 0)) and b"another size" in says(lib, resident=(16, 16), fmt=(1, 0))
    for side, ok in ((15, False), (16, True), (8192, True), (8193, False)):
        assert (says(lib, source=(side, 123), fmt=(0, 0)) is None) == ok and (says(lib, source=(161, side)) is None) == ok
        assert (says(lib, source=(side, 123), fmt=None) is None) == ok
    for enc, ok in ((-1, False), (0, True), (1, False), (2, True), (3, True), (4, True), (5, True), (6, True), (7, True), (8, False)):
        assert (says(lib, fmt=(enc, 0)) is None) == ok
    # bgr8: a source row is 483 bytes, a row of the tracked image 393: the step is judged beside the source
    for step, ok in ((-1, False), (0, True), (393, False), (482, False), (483, True), (487, True), (65536, True), (65537, False)):
        assert (says(lib, fmt=(2, step)) is None) == ok, step
    assert says(lib, fmt=(0, 160)) is not None and says(lib, fmt=(0, 161)) is None
    out = np.zeros(6, np.int64)
    for fmt, want in ((None, (123 * 161, 161, 123, 161, 1, 0)), ((2, 0), (123 * 483, 161, 123, 483, 3, 2)), ((2, 487), (123 * 487, 161, 123, 487, 3, 2)),
                      ((7, 325), (123 * 325, 161, 123, 325, 2, 7)), ((4, 0), (123 * 644, 161, 123, 644, 4, 4))):
        enc, step = fmt or (0, 0)
        lib.ts_plan(161, 123, fmt is None, enc, step, _p(out, C.c_longlong))
        assert tuple(out.tolist()) == want and out[0] == ts.upload_bytes((161, 123), fmt), fmt
    assert ts.set_check(15, 123) and ts.set_check(161, 8193) and not ts.set_check(16, 8192)


# ---- 2
SW, SH = 161, 123
CAM = pr.small(pr.PAL, pr.CAMS["PAL"][1][0] / SW)
EUROC_ND = pr.small(pr.CAMS["EUROC_ND"][0], pr.CAMS["EUROC_ND"][1][0] / SW)


def shifted_M(cam, dx, dy):
    """K^-1 of a pinhole camera behind a shift of the output pixel: part of the output looks outside the source."""
    return pr.K_inverse(cam) @ np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def maps():
    """(kind, W, H) -> float maps; computed once, shared, never changed."""
    out = {}
    for W, H in ((131, 67), (128, 64)):
        out["equirect", W, H] = pr.build(CAM, pr.MAP_EQUIRECT, W, H)
        out["perspective", W, H] = pr.build(EUROC_ND, pr.MAP_PERSPECTIVE, W, H, shifted_M(EUROC_ND, -20.0, 70.0))
    return out


@pytest.mark.parametrize("size", ((131, 67), (128, 64)))
@pytest.mark.parametrize("kind", ("equirect", "perspective"))
def test_lane_equals_gray_of_remap(lib, maps, kind, size):
    W, H = size
    n = W * H
    assert (n % 4 == 1) == (size == (131, 67))
    mx, my = maps[kind, W, H]
    counts, runs = np.zeros(2, np.int64), 0
    for enc in ir.CODES:
        for step in (0, SW * ir.BPP[enc] + 5 + ir.BPP[enc] % 2):  # (the padded step is odd: 167, 327, 489, 649)
            src = pr.noise_image(enc * 10 + (step > 0), SW, SH, enc, step)
            got = np.full(n + 64, 0xEE, np.uint8)
            lanes = lib.ts_level0(enc, step, SW, SH, n, _p(mx, C.c_float), _p(my, C.c_float), _p(src, C.c_ubyte), _p(got, C.c_ubyte), _p(counts, C.c_longlong))
            assert lanes == ts.lanes(n) and lanes * 4 >= n
            assert counts[0] > n // 10 and counts[1] > n // 10 and counts.sum() == n, counts  # the gather and the select both run
            want = ts.level0(src, mx, my, SW, SH, enc, step)
            assert want.shape == (H, W) and np.array_equal(got[:n].reshape(H, W), want), (enc, step)
            assert np.all(got[n:] == 0xEE)
            zero = np.unique(want[pr.offsets(mx, my, SW, SH, step or SW * ir.BPP[enc], ir.BPP[enc]) < 0])
            assert step == 0 or step % 2 == 1
            assert zero.tolist() == [0]  # the grey value of a zero pixel, in every encoding
            runs += 1
    assert runs == 14


# ---- 3
def test_launch_geometry(lib):
    out = np.zeros(2, np.int64)
    for n in (256, 257, 1024, 1025, 131 * 67, 128 * 64, 960 * 480, 8192 * 8192):
        lib.ts_geometry(n, _p(out, C.c_longlong))
        blocks = -(-(-(-n // 4)) // 256)
        assert out.tolist() == [blocks, blocks * 256] and out[1] == ts.lanes(n) and out[1] * 4 >= n and (blocks - 1) * 1024 < n
