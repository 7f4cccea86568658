"""CPU tests of lf-vio_amd/csrc/trackbatch_source_plan.h and the TbMaps part of trackbatch_plan.h — the plain C++ behind
lfvio_track_batch_map / lfvio_track_batch_source — compiled alone with g++ -ffp-contract=off -Wall -Werror behind a
ctypes shim.

  1  the per-call check refuses each case with a message of its own, each beside a neighbour that is accepted: an active slot with no
     map, an active slot whose map is of another size than width x height, a step one byte short of src_width * bytes per pixel
     (judged beside the SOURCE's width), source sides of 15 and 8193 (at the set call and at the frame call); idle slots need no map;
     the setting off judges nothing; the maps come before the format
  2  the per-slot layout of the maps: 12 bytes per output pixel before alignment, every plane of every slot 256-aligned for W x H =
     131 x 67, 128 x 64 and 17 x 16 and slots = 1, 3, 64, planes that do not overlap, a grown layout that covers both; level 0 of
     either pyramid buffer of every slot 4-aligned at the same sizes
  3  the rebuild decision equals remap_needs_index for every pair of geometries of a list (width, height, step, bytes per pixel
     changed one at a time) and for a record that was never written; a build writes for the record's geometry, or for none
  4  the host copy of one lane of k_remap_gray_b: three slots with three different maps in one block laid out by TbMaps, every lane of
     the launch per slot equals tracksource_ref.level0 of that slot's own map; guard bytes behind level 0 stay
  5  tests/tools/track_batch_source_walk.cpp, a stand-alone program, builds with -fsanitize=address,undefined and runs clean"""
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
CSRC = os.path.join(ROOT, "lf-vio_amd", "csrc")

SRC = r'''
#include <cstring>
#include <vector>

#include "trackbatch_source_plan.h"
// slots entries: active[i], map_valid[i], map_w[i], map_h[i]; every active entry is W x H
extern "C" const char *tbs_check(int on, int sw, int sh, int null_fmt, int encoding, int step, int slots, const int *active, const int *valid, const int *mw,
                                 const int *mh, int W, int H) {
  TrackSourceState s;
  s.on = on != 0, s.sw = sw, s.sh = sh;
  static const unsigned char pixel = 0;
  std::vector<LfvioTrackFrameIn> in((size_t)slots);
  std::vector<TbMapInfo> maps((size_t)slots);
  for (int i = 0; i < slots; i++) {
    std::memset(&in[i], 0, sizeof in[i]);
    in[i].image = active[i] ? &pixel : nullptr, in[i].width = W, in[i].height = H;
    maps[i].valid = valid[i] != 0, maps[i].width = mw[i], maps[i].height = mh[i];
  }
  const LfvioImageFormat f = {encoding, step};
  return trackbatch_source_check(s, null_fmt ? nullptr : &f, slots, in.data(), maps.data());
}
extern "C" const char *tbs_set_check(int sw, int sh) { return trackbatch_source_set_check(sw, sh); }
extern "C" const char *tbs_level_check(int slot, int slots, int resident, int level, int built) { return trackbatch_level_check(slot, slots, resident != 0, level, built); }
// out: px, plane, x_at, y_at, index_at, stride, aligned(slots), level0_aligned(slots), image stride
extern "C" void tbs_layout(int W, int H, int slots, long long *out) {
  const TbMaps m = trackbatch_maps(W, H);
  out[0] = (long long)m.px, out[1] = (long long)m.plane(), out[2] = (long long)m.x_at(), out[3] = (long long)m.y_at(), out[4] = (long long)m.index_at();
  out[5] = (long long)m.stride(), out[6] = trackbatch_maps_aligned(m, slots);
  const TbImage lay = trackbatch_image(W, H, gft_work(W, H).bytes);
  out[7] = trackbatch_level0_aligned(lay, slots), out[8] = (long long)lay.stride();
}
extern "C" int tbs_grown(int W0, int H0, int W1, int H1, long long *out) {
  const TbMaps a = trackbatch_maps(W0, H0), b = trackbatch_maps(W1, H1), g = trackbatch_maps_grown(a, b);
  out[0] = (long long)g.px;
  return trackbatch_maps_covers(g, a) && trackbatch_maps_covers(g, b) && (trackbatch_maps_covers(a, b) == (a.px >= b.px));
}
static RemapGeom geom(const int *g) { return RemapGeom{g[0], g[1], g[2], g[3]}; }
// -> (trackbatch_needs_index, remap_needs_index) as bits 0 and 1; build: the geometry a build writes for, 4 ints
extern "C" int tbs_needs(int indexed, const int *have, const int *now, int *build) {
  TbIndexed r;
  r.indexed = indexed != 0, r.geom = geom(have);
  RemapResident one;
  one.valid = true, one.indexed = indexed != 0, one.geom = geom(have);
  const RemapGeom b = trackbatch_build_geom(r);
  build[0] = b.sw, build[1] = b.sh, build[2] = b.step, build[3] = b.bpp;
  return (trackbatch_needs_index(r, geom(now)) ? 1 : 0) | (remap_needs_index(one, geom(now)) ? 2 : 0);
}
// slot `slot`'s integer map written into the block `maps` (slots * stride bytes) from float maps, then every lane for that slot
extern "C" long long tbs_level0(int encoding, int step, int sw, int sh, int W, int H, int capW, int capH, int slot, char *maps, const float *mx, const float *my,
                                const unsigned char *src, unsigned char *level0) {
  const TbMaps lay = trackbatch_maps(capW, capH);
  const LfvioImageFormat f = {encoding, step};
  const RemapGeom g = remap_geom(f, sw, sh);
  const size_t pixels = (size_t)W * H;
  int *imap = (int *)(maps + (size_t)slot * lay.stride() + lay.index_at());
  for (size_t p = 0; p < pixels; p++) imap[p] = remap_offset(mx[p], my[p], g);
  if (trackbatch_slot_index(maps, lay, slot) != imap) return -1;
  const size_t lanes = tracksource_lanes(pixels);
  for (size_t lane = 0; lane < lanes; lane++) trackbatch_source_lane(encoding, maps, lay, slot, src, level0, pixels, lane);
  return (long long)lanes;
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="trackbatch_source_plan_")
    src, so = os.path.join(d, "tbs.cpp"), os.path.join(d, "libtbs.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, src, "-o", so])
    so = C.CDLL(so)
    i, ll, ip, fp, up, lp = C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)
    so.tbs_check.restype, so.tbs_check.argtypes = C.c_char_p, [i] * 7 + [ip] * 4 + [i, i]
    so.tbs_set_check.restype, so.tbs_set_check.argtypes = C.c_char_p, [i, i]
    so.tbs_level_check.restype, so.tbs_level_check.argtypes = C.c_char_p, [i] * 5
    so.tbs_layout.restype, so.tbs_layout.argtypes = None, [i, i, i, lp]
    so.tbs_grown.restype, so.tbs_grown.argtypes = i, [i] * 4 + [lp]
    so.tbs_needs.restype, so.tbs_needs.argtypes = i, [i, ip, ip, ip]
    so.tbs_level0.restype, so.tbs_level0.argtypes = ll, [i] * 9 + [C.c_char_p, fp, fp, up, up]
    return so


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


W, H = 131, 67
SW, SH = 161, 123


def says(lib, slots, source=(SW, SH), fmt=(2, 0), size=(W, H)):
    """slots: per slot (active, map) with map None or (width, height)."""
    on, (sw, sh) = source is not None, source or (0, 0)
    enc, step = fmt or (0, 0)
    a = np.array([int(s[0]) for s in slots], np.int32)
    v = np.array([int(s[1] is not None) for s in slots], np.int32)
    mw = np.array([(s[1] or (0, 0))[0] for s in slots], np.int32)
    mh = np.array([(s[1] or (0, 0))[1] for s in slots], np.int32)
    return lib.tbs_check(on, sw, sh, fmt is None, enc, step, len(slots), _p(a, C.c_int), _p(v, C.c_int), _p(mw, C.c_int), _p(mh, C.c_int), size[0], size[1])


# ---- 1
def test_call_check(lib):
    good = [(True, (W, H))] * 3
    assert says(lib, good) is None and says(lib, good, fmt=None) is None and says(lib, good, fmt=(2, 487)) is None
    # idle slots need no map, and an idle slot's map may be of any size
    assert says(lib, [(True, (W, H)), (False, None), (False, (128, 64))]) is None
    assert says(lib, [(False, None)] * 3) is None
    # the setting off judges nothing
    assert says(lib, [(True, None)] * 2, source=None, fmt=(9, -1)) is None
    no_map = says(lib, [(True, (W, H)), (True, None), (True, (W, H))])
    other = says(lib, [(True, (W, H)), (True, (W, H)), (True, (128, 64))])
    short = says(lib, good, fmt=(2, 3 * SW - 1))
    side = says(lib, good, source=(15, SH))
    assert b"no map" in no_map and b"another size" in other and b"step below width" in short and b"[16, 8192]" in side
    assert len({no_map, other, short, side}) == 4  # each its own message
    for bad in ((130, 67), (131, 66), (67, 131), (SW, SH)):
        assert b"another size" in says(lib, [(True, bad)])
    # the step is judged beside the source: enough for the 131 pixels tracked is not enough for 161
    for step, ok in ((0, True), (3 * W, False), (3 * SW - 1, False), (3 * SW, True), (3 * SW + 4, True), (65536, True), (65537, False)):
        assert (says(lib, good, fmt=(2, step)) is None) == ok, step
    assert says(lib, good, fmt=(0, SW - 1)) is not None and says(lib, good, fmt=(0, SW)) is None and says(lib, good, fmt=None) is None
    for s, ok in ((15, False), (16, True), (8192, True), (8193, False)):
        assert (says(lib, good, source=(s, SH), fmt=(0, 0)) is None) == ok and (says(lib, good, source=(SW, s), fmt=None) is None) == ok
        assert (lib.tbs_set_check(s, SH) is None) == ok and (lib.tbs_set_check(SW, s) is None) == ok and ts.set_check(s, SH) == (not ok)
    # the maps before the format
    assert b"no map" in says(lib, [(True, None)], fmt=(1, 0)) and b"another size" in says(lib, [(True, (16, 16))], fmt=(1, 0))
    assert says(lib, good, fmt=(1, 0)) is not None


def test_level_check(lib):
    """lfvio_track_batch_level's arguments: one slot of the reserved ones (never -1), a resident image, a level some call built."""
    assert lib.tbs_level_check(0, 3, 1, 0, 3) is None and lib.tbs_level_check(2, 3, 1, 3, 3) is None and lib.tbs_level_check(0, 1, 1, 0, 0) is None
    for slot, slots in ((-1, 3), (3, 3), (0, 0), (64, 64), (-2, 3)):
        assert b"slot outside" in lib.tbs_level_check(slot, slots, 1, 0, 3), (slot, slots)
    assert b"no resident image" in lib.tbs_level_check(1, 3, 0, 0, 3)
    for level, built in ((-1, 3), (4, 3), (1, 0), (6, 5)):
        assert b"not built" in lib.tbs_level_check(1, 3, 1, level, built), (level, built)
    assert b"slot outside" in lib.tbs_level_check(3, 3, 0, 9, 0)  # the slot first


# ---- 2
@pytest.mark.parametrize("slots", (1, 3, 64))
@pytest.mark.parametrize("size", ((131, 67), (128, 64), (17, 16)))
def test_map_layout(lib, size, slots):
    out = np.zeros(9, np.int64)
    lib.tbs_layout(size[0], size[1], slots, _p(out, C.c_longlong))
    px, plane, x_at, y_at, index_at, stride, aligned, level0_aligned, image_stride = out.tolist()
    assert px == size[0] * size[1] and plane >= 4 * px and plane - 4 * px < 256 and plane % 256 == 0
    assert (x_at, y_at, index_at, stride) == (0, plane, 2 * plane, 3 * plane)  # 12 bytes per output pixel, aligned
    assert aligned == 1 and level0_aligned == 1 and image_stride % 256 == 0
    for slot in range(slots):
        for at in (x_at, y_at, index_at):
            assert (slot * stride + at) % 256 == 0
    assert slots * stride < 2 ** 31


def test_map_layout_grows(lib):
    out = np.zeros(1, np.int64)
    for a, b in (((131, 67), (128, 64)), ((128, 64), (131, 67)), ((17, 16), (17, 16)), ((16, 16), (8192, 8192))):
        assert lib.tbs_grown(a[0], a[1], b[0], b[1], _p(out, C.c_longlong)) == 1
        assert out[0] == max(a[0] * a[1], b[0] * b[1])


# ---- 3
def test_rebuild_decision(lib):
    base = (1280, 960, 3840, 3)
    geoms = [base, (1281, 960, 3843, 3), (1280, 961, 3840, 3), (1280, 960, 3844, 3), (1280, 960, 5120, 4), (1280, 960, 1280, 1), (161, 123, 489, 3)]
    build = np.zeros(4, np.int32)
    for have in geoms:
        for now in geoms:
            a, b = np.array(have, np.int32), np.array(now, np.int32)
            got = lib.tbs_needs(1, _p(a, C.c_int), _p(b, C.c_int), _p(build, C.c_int))
            assert got == (3 if have != now else 0), (have, now)
            assert tuple(build.tolist()) == have  # a later build writes its integer map for the record's geometry
        # never written: every geometry needs it, the one in the record too, and a build writes no integer map
        a = np.array(have, np.int32)
        assert lib.tbs_needs(0, _p(a, C.c_int), _p(a, C.c_int), _p(build, C.c_int)) == 3 and build.tolist() == [0, 0, 0, 0]


# ---- 4
def shifted_M(cam, dx, dy):
    return pr.K_inverse(cam) @ np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("size", ((131, 67), (128, 64)))
def test_lane_per_slot(lib, size):
    w, h = size
    n = w * h
    pal = pr.small(pr.PAL, pr.CAMS["PAL"][1][0] / SW)
    pal2 = pr.small(pr.PAL, 1.15 * pr.CAMS["PAL"][1][0] / SW)
    pin = pr.small(pr.CAMS["EUROC_ND"][0], pr.CAMS["EUROC_ND"][1][0] / SW)
    maps = [pr.build(pal, pr.MAP_EQUIRECT, w, h), pr.build(pin, pr.MAP_PERSPECTIVE, w, h, shifted_M(pin, -20.0, 70.0)), pr.build(pal2, pr.MAP_EQUIRECT, w, h)]
    cap = (131, 67)  # the block's capacity: the largest map
    out = np.zeros(9, np.int64)
    lib.tbs_layout(cap[0], cap[1], 3, _p(out, C.c_longlong))
    stride = int(out[5])
    runs = 0
    for enc in (ir.MONO8, ir.BGR8, ir.BGRA8, ir.MONO16, ir.MONO16_BE):
        step = SW * ir.BPP[enc] + 5 + ir.BPP[enc] % 2
        assert step % 2 == 1
        src = pr.noise_image(90 + enc, SW, SH, enc, step)
        block = C.create_string_buffer(3 * stride)  # exactly the three slots' maps
        levels = []
        for slot, (mx, my) in enumerate(maps):
            got = np.full(n + 64, 0xEE, np.uint8)
            lanes = lib.tbs_level0(enc, step, SW, SH, w, h, cap[0], cap[1], slot, block, _p(mx, C.c_float), _p(my, C.c_float), _p(src, C.c_ubyte), _p(got, C.c_ubyte))
            assert lanes == ts.lanes(n)
            want = ts.level0(src, mx, my, SW, SH, enc, step)
            off = pr.offsets(mx, my, SW, SH, step, ir.BPP[enc])
            assert (off >= 0).any() and (off < 0).any()
            assert np.array_equal(got[:n].reshape(h, w), want) and np.all(got[n:] == 0xEE), (enc, slot)
            levels.append(want.tobytes())
            runs += 1
        assert len(set(levels)) == 3  # three maps, not one
    assert runs == 15


# ---- 5
def test_walk_under_the_sanitizers():
    d = tempfile.mkdtemp(prefix="track_batch_source_walk_")
    exe = os.path.join(d, "track_batch_source_walk")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "tools", "track_batch_source_walk.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "0 wrong" in r.stdout, r.stdout + r.stderr
