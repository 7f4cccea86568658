"""CPU tests of the host side of lfvio_track_batch_* that needs no device (lf-vio_amd/csrc/trackbatch_plan.h, compiled alone with
g++) and of the ABI names.

  1  every refusal: count != slots, a disagreeing field (each of the fourteen in turn), a per-entry refusal in one slot only, a
     capacity below one slot's count, slots outside [0, 64], a slot index outside its range; an all-idle call is accepted
  2  the bounds n0_max and B_max
  3  the staging layout: no two segments overlap, with mixed publish flags and with idle slots, and slot i's down segments lie where
     the host reads them, inside the one range that comes down
  4  the bytes one slot owns at an image size; a layout only grows
  5  the five names are in the header, in abi.HIP_SYMBOLS and in the built library"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import track_frame_ref as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INT_KEYS = ("width", "height", "publish", "win_size", "max_level", "max_iterations", "border", "max_count", "min_distance", "mask_radius", "num_samples",
            "capacity")
DBL_KEYS = ("time", "epsilon", "min_eig_threshold", "quality_level")
SHARED = ("width", "height", "win_size", "max_level", "max_iterations", "epsilon", "min_eig_threshold", "border", "max_count", "quality_level",
          "min_distance", "mask_radius", "num_samples", "capacity")
STAGE = ("desc", "words", "images", "in_end", "mid", "mid_stride", "down", "down_stride", "end", "c1", "t1", "t2", "bl", "br", "A", "score", "E", "raw",
         "matched", "next", "status", "samples", "mask", "kept", "corners", "dev", "table", "un", "un3d", "vel", "msg")

SRC = r'''
#include "trackbatch_plan.h"
// entry i: iv[15 i ..] = the twelve ints of tests/test_track_frame_ref.py, active, camera model (-1: null), have_words; dv[4 i ..]
static void fill(int count, const int *iv, const double *dv, LfvioTrackFrameIn *in, LfvioCamera *cam) {
  static const unsigned char px = 0;
  static const unsigned words[8] = {0};
  for (int i = 0; i < count; i++, iv += 15, dv += 4) {
    cam[i] = LfvioCamera{};
    cam[i].model = iv[13], cam[i].c = 1.0;
    LfvioTrackFrameIn &e = in[i];
    e = LfvioTrackFrameIn{};
    e.width = iv[0], e.height = iv[1], e.publish = iv[2], e.win_size = iv[3], e.max_level = iv[4], e.max_iterations = iv[5];
    e.border = iv[6], e.max_count = iv[7], e.min_distance = iv[8], e.mask_radius = iv[9], e.num_samples = iv[10], e.capacity = iv[11];
    e.time = dv[0], e.epsilon = dv[1], e.min_eig_threshold = dv[2], e.quality_level = dv[3];
    e.image = iv[12] ? &px : nullptr, e.camera = iv[13] >= 0 ? &cam[i] : nullptr, e.sample_words = iv[14] ? words : nullptr;
  }
}
extern "C" const char *tbp_frame_check(int slots, int count, const int *iv, const double *dv, const int *table_counts) {
  LfvioTrackFrameIn in[80];
  LfvioCamera cam[80];
  fill(count, iv, dv, in, cam);
  return trackbatch_frame_check(slots, count, in, table_counts);
}
extern "C" void tbp_bounds(int count, const int *iv, const double *dv, const int *table_counts, int *out) {
  LfvioTrackFrameIn in[80];
  LfvioCamera cam[80];
  fill(count, iv, dv, in, cam);
  const TbBounds b = trackbatch_bounds(count, in, table_counts);
  out[0] = b.active, out[1] = b.publishing, out[2] = b.first, out[3] = b.n0_max, out[4] = b.B_max;
}
extern "C" const char *tbp_reserve_check(int slots) { return trackbatch_reserve_check(slots); }
extern "C" const char *tbp_slot_check(int slot, int slots) { return trackbatch_slot_check(slot, slots); }
static TbShape shape_of(const unsigned long long *s) {
  TbShape v = {};
  v.slots = (int)s[0], v.publishing = (int)s[1], v.active = (int)s[2];
  v.n0_max = s[3], v.B_max = s[4], v.S = s[5], v.max_count = s[6], v.pixels = s[7], v.dev_bytes = s[8], v.rows = s[9] != 0;
  return v;
}
extern "C" int tbp_stage(const unsigned long long *s, unsigned long long *out) {
  const TbStage o = trackbatch_stage(shape_of(s));
  const size_t v[] = {o.desc, o.words, o.images, o.in_end, o.mid, o.mid_stride, o.down, o.down_stride, o.end, o.c1, o.t1, o.t2, o.bl, o.br, o.A, o.score,
                      o.E, o.raw, o.matched, o.next, o.status, o.samples, o.mask, o.kept, o.corners, o.dev, o.table, o.un, o.un3d, o.vel, o.msg};
  const int n = (int)(sizeof v / sizeof v[0]);
  for (int k = 0; k < n; k++) out[k] = v[k];
  return n;
}
// which: 0 the k-th publishing slot's words, 1 the k-th active slot's image, 2 slot k's mid segment, 3 slot k's down segment
extern "C" unsigned long long tbp_at(const unsigned long long *s, int which, int k) {
  const TbShape v = shape_of(s);
  const TbStage o = trackbatch_stage(v);
  return which == 0 ? trackbatch_words_at(o, v, k) : which == 1 ? trackbatch_image_at(o, v, k) : which == 2 ? trackbatch_mid_at(o, k) : trackbatch_down_at(o, k);
}
extern "C" void tbp_image(int w, int h, unsigned long long work, unsigned long long *out) {
  const TbImage m = trackbatch_image(w, h, (size_t)work);
  out[0] = m.pyr, out[1] = m.mask, out[2] = m.work, out[3] = m.stride(), out[4] = trackbatch_slot_bytes(w, h, (size_t)work), out[5] = TB_FIXED_BYTES;
  out[6] = m.pyr_at(1), out[7] = m.mask_at(), out[8] = m.work_at(), out[9] = klt_plan(w, h, 0, LFVIO_KLT_MAX_LEVEL).bytes;
  // beside a wider image with smaller arrays: every segment the larger of the two
  const TbImage wide = trackbatch_image(2 * w, h, (size_t)work / 2), g = trackbatch_image_grown(m, wide);
  out[10] = g.pyr, out[11] = g.mask, out[12] = g.work;
  out[13] = trackbatch_image_covers(g, m) && trackbatch_image_covers(g, wide) && !trackbatch_image_covers(m, g) && !trackbatch_image_covers(wide, m);
}
extern "C" int tbp_sizes(int *out) {
  out[0] = (int)sizeof(TbSlot), out[1] = LFVIO_TRACK_BATCH_MAX_SLOTS, out[2] = (int)TB_ALIGN;
  return 3;
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="trackbatch_plan_")
    src, so = os.path.join(d, "tbp.cpp"), os.path.join(d, "libtbp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    ip, dp, up = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
    so.tbp_frame_check.restype = C.c_char_p
    so.tbp_frame_check.argtypes = [C.c_int, C.c_int, ip, dp, ip]
    so.tbp_bounds.restype = None
    so.tbp_bounds.argtypes = [C.c_int, ip, dp, ip, ip]
    so.tbp_reserve_check.restype = so.tbp_slot_check.restype = C.c_char_p
    so.tbp_stage.argtypes = [up, up]
    so.tbp_at.restype = C.c_ulonglong
    so.tbp_at.argtypes = [up, C.c_int, C.c_int]
    so.tbp_image.restype = None
    so.tbp_image.argtypes = [C.c_int, C.c_int, C.c_ulonglong, up]
    return so


GOOD = dict(tf.DEFAULTS, width=161, height=123, num_samples=100, capacity=150, publish=1, time=1.0, active=1, cam_model=0, have_words=1)


def pack(entries):
    iv, dv = [], []
    for e in entries:
        e = dict(GOOD, active=0) if e is None else e
        iv += [int(e[k]) for k in INT_KEYS] + [e["active"], e["cam_model"], e["have_words"]]
        dv += [float(e[k]) for k in DBL_KEYS]
    return (C.c_int * len(iv))(*iv), (C.c_double * len(dv))(*dv)


def says(lib, entries, counts=None, slots=None, count=None):
    n = len(entries)
    iv, dv = pack(entries)
    tc = (C.c_int * max(n, 1))(*(counts or [0] * n))
    return lib.tbp_frame_check(n if slots is None else slots, n if count is None else count, iv, dv, tc)


def test_every_refusal(lib):
    three = [GOOD, GOOD, GOOD]
    assert says(lib, three) is None
    # count != slots, no slots
    for slots, count in ((3, 2), (2, 3), (3, 0), (0, 0), (0, 3)):
        assert says(lib, three[:max(count, 1)] if count else three, slots=slots, count=count) is not None, (slots, count)
    # a disagreeing field, each of the fourteen in turn, every value valid on its own; in any slot but not in an idle one
    other = dict(width=160, height=122, win_size=39, max_level=2, max_iterations=29, epsilon=0.02, min_eig_threshold=2e-4, border=2, max_count=149,
                 quality_level=0.02, min_distance=29, mask_radius=29, num_samples=99, capacity=151)
    assert tuple(other) == SHARED and len(SHARED) == 14
    for key, v in other.items():
        odd = dict(GOOD, **{key: v})
        assert says(lib, [odd]) is None and says(lib, [odd, odd, odd]) is None, key
        for at in range(3):
            entries = [odd if k == at else GOOD for k in range(3)]
            why = says(lib, entries)
            assert why is not None and why.startswith(b"lfvio_track_batch_frame: active entries of different"), (key, at, why)
            assert says(lib, [dict(odd, active=0) if k == at else GOOD for k in range(3)]) is None, (key, at)
    # what may differ
    for key, v in (("time", 7.0), ("publish", 0), ("have_words", 0)):
        free = dict(GOOD, **{key: v}) if key != "have_words" else dict(GOOD, publish=0, have_words=0)
        assert says(lib, [GOOD, free, GOOD]) is None, key
    # a per-entry refusal in one slot only: what trackframe_check says of that entry
    nan = float("nan")
    for bad in (dict(win_size=4), dict(max_level=6), dict(epsilon=nan), dict(num_samples=0), dict(cam_model=-1), dict(cam_model=1), dict(have_words=0),
                dict(time=nan), dict(quality_level=0.0), dict(max_count=0), dict(width=15)):
        for at in range(3):
            why = says(lib, [dict(GOOD, **bad) if k == at else GOOD for k in range(3)])
            assert why is not None and not why.startswith(b"lfvio_track_batch_frame: active"), (bad, at, why)
            assert says(lib, [dict(GOOD, active=0, **bad) if k == at else GOOD for k in range(3)]) is None, (bad, at)
    # a capacity below one slot's count
    assert says(lib, three, counts=[150, 150, 150]) is None
    for at in range(3):
        counts = [151 if k == at else 10 for k in range(3)]
        assert says(lib, three, counts=counts) is not None, at
        assert says(lib, [None if k == at else GOOD for k in range(3)], counts=counts) is None, at  # the slot is idle: its count does not matter
        assert says(lib, [dict(GOOD, capacity=151)] * 3, counts=counts) is None, at
    # an all-idle call is accepted
    assert says(lib, [None, None, None], counts=[5, 200, 0]) is None
    out = (C.c_int * 5)()
    iv, dv = pack([None, None, None])
    lib.tbp_bounds(3, iv, dv, (C.c_int * 3)(5, 200, 0), out)
    assert list(out) == [0, 0, -1, 0, 0]
    # slots outside [0, 64]; a slot index outside its range for mask and reset
    for slots in (-1, 65, 1000):
        assert lib.tbp_reserve_check(slots) is not None
    for slots in (0, 1, 64):
        assert lib.tbp_reserve_check(slots) is None
    for slot, slots, ok in ((-1, 3, True), (0, 3, True), (2, 3, True), (3, 3, False), (-2, 3, False), (0, 0, False), (-1, 0, False), (63, 64, True), (64, 64, False)):
        assert (lib.tbp_slot_check(slot, slots) is None) == ok, (slot, slots)


def test_bounds(lib):
    quiet = dict(GOOD, publish=0, have_words=0)
    cases = [([GOOD, GOOD, GOOD], [0, 0, 0], [3, 3, 0, 0, 150]), ([GOOD, quiet, None], [10, 200, 4000], [2, 1, 0, 200, 200]),
             ([None, quiet, quiet], [4000, 20, 30], [2, 0, 1, 30, 30]), ([None, None, GOOD], [7, 7, 160], [1, 1, 2, 160, 160]),
             ([quiet, GOOD], [149, 3], [2, 1, 0, 149, 150]), ([quiet], [0], [1, 0, 0, 0, 0])]
    for entries, counts, want in cases:
        iv, dv = pack(entries)
        out = (C.c_int * 5)()
        lib.tbp_bounds(len(entries), iv, dv, (C.c_int * len(counts))(*counts), out)
        assert list(out) == want, (counts, list(out))


def stage(lib, **s):
    keys = ("slots", "publishing", "active", "n0_max", "B_max", "S", "max_count", "pixels", "dev_bytes", "rows")
    arr = (C.c_ulonglong * 10)(*[int(s[k]) for k in keys])
    out = (C.c_ulonglong * 40)()
    n = lib.tbp_stage(arr, out)
    assert n == len(STAGE)
    return dict(zip(STAGE, list(out)[:n])), arr


@pytest.mark.parametrize("slots,flags", [(1, "P"), (3, "PPP"), (3, "PQ-"), (4, "-Q-P"), (5, "QQQQQ"), (64, "P-Q" * 21 + "P")])
@pytest.mark.parametrize("n0_max,B_max,rows", [(0, 40, 1), (150, 150, 1), (37, 40, 0), (4096, 4096, 1), (0, 0, 1)])
def test_staging_layout(lib, slots, flags, n0_max, B_max, rows):
    """flags: P an active slot that publishes, Q one that does not, - an idle one."""
    S, MC, px, dev = 100, 40, 161 * 123, 136
    active, pub = sum(f != "-" for f in flags), flags.count("P")
    o, arr = stage(lib, slots=slots, publishing=pub, active=active, n0_max=n0_max, B_max=B_max, S=S, max_count=MC, pixels=px, dev_bytes=dev, rows=rows)
    sizes = lib_sizes(lib)
    seg = [(o["desc"], slots * sizes[0], "desc")]
    seg += [(lib.tbp_at(arr, 0, k), S * 32, ("words", k)) for k in range(pub)] + [(lib.tbp_at(arr, 1, k), px, ("image", k)) for k in range(active)]
    assert all(a + n <= o["in_end"] for a, n, _ in seg) and o["in_end"] <= o["mid"]
    N0, B = n0_max, B_max
    mid = dict(c1=N0 * 8, t1=N0 * 16, t2=N0 * 16, bl=N0 * 24, br=N0 * 24, A=max(N0, 9) * 72, score=S * 4, E=S * 72, raw=B * 4, matched=B * 4, next=N0 * 8,
               status=N0, samples=S * 32, mask=N0, kept=N0 * 4, corners=MC * 8)
    down = dict(dev=dev, table=B * 16, un=B * 8, un3d=B * 12, vel=B * 12)
    if rows:
        down["msg"] = 16 + B * 36
    for i in range(slots):
        m, d = lib.tbp_at(arr, 2, i), lib.tbp_at(arr, 3, i)
        assert m == o["mid"] + i * o["mid_stride"] and d == o["down"] + i * o["down_stride"]
        seg += [(m + o[k], n, (i, k)) for k, n in mid.items()] + [(d + o[k], n, (i, k)) for k, n in down.items()]
        # where the host reads slot i: inside the one range that comes down, [down, end)
        for k, n in down.items():
            assert o["down"] <= d + o[k] and d + o[k] + n <= o["end"], (i, k)
        assert all(o[k] + n <= o["mid_stride"] for k, n in mid.items()) and all(o[k] + n <= o["down_stride"] for k, n in down.items())
    assert o["down"] == o["mid"] + slots * o["mid_stride"] and o["end"] == o["down"] + slots * o["down_stride"]
    live = sorted((a, n, tag) for a, n, tag in seg if n)
    for (a, n, ta), (b, _, tb_) in zip(live, live[1:]):
        assert a + n <= b, (ta, tb_)
    assert all(a % sizes[2] == 0 for a, _, _ in seg) and live[-1][0] + live[-1][1] <= o["end"]


def lib_sizes(lib):
    v = (C.c_int * 3)()
    assert lib.tbp_sizes(v) == 3
    return list(v)


def test_slot_bytes_and_growth(lib):
    sizes = lib_sizes(lib)
    assert sizes[1] == 64 and sizes[0] % 8 == 0
    for w, h, work in ((161, 123, 300000), (1280, 960, 16 << 20), (16, 16, 0), (8192, 8192, 1 << 30)):
        out = (C.c_ulonglong * 14)()
        lib.tbp_image(w, h, work, out)
        pyr, mask, wk, stride, total, fixed, p1, m_at, w_at, plan_bytes, gp, gm, gw, covers = list(out)
        assert pyr >= plan_bytes and mask >= w * h and wk >= work and all(v % sizes[2] == 0 for v in (pyr, mask, wk))
        assert (p1, m_at, w_at, stride) == (pyr, 2 * pyr, 2 * pyr + mask, 2 * pyr + mask + wk)
        assert fixed == 2 * 4096 * 16 + 2 * 4096 * 16 and total == fixed + stride
        assert gp > pyr and gm > mask and gw == wk and covers == (1 if work else 0)  # (work = 0: the wider image covers)


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi
    from lfvio.engine import Engine

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("reserve", "set_mask", "clahe", "frame", "reset"):
        full = "lfvio_track_batch_" + name
        assert re.search(r"\bint\s+%s\s*\(" % full, src), full
        assert full in abi.HIP_SYMBOLS and hasattr(lib, full), full
        assert callable(getattr(Engine, "track_batch_" + name)), name
    assert re.search(r"#define\s+LFVIO_TRACK_BATCH_MAX_SLOTS\s+64\b", src)
