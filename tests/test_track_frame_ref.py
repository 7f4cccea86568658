"""CPU tests of lfvio_track_frame's specification (tests/track_frame_ref.py), its host-side checks (lf-vio_amd/csrc/trackframe_plan.h,
compiled alone with g++) and the ABI names.

  1  draw() against a brute-force "k-th of the remaining indices" restatement at n = 8, 9, 64 and 4096; at n = 8 every set is a
     permutation of 0 .. 7; the indices are distinct and in range; the words 0 and 0xFFFFFFFF
  2  trackframe_draw of the header gives draw()'s indices
  3  trackframe_plan.h refuses what track_frame_ref.check refuses, field by field
  4  a frame of the restatement on a small image: the table's invariants
  5  the two names are in the header, in abi.HIP_SYMBOLS and in the built library"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import klt_ref
import track_frame_ref as tf
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(words, n):
    out = np.zeros(words.shape, np.int32)
    for s, row in enumerate(words):
        left = list(range(n))
        for k in range(8):
            out[s, k] = left.pop(int(row[k]) % len(left))
    return out


def words_for(seed, S):
    w = np.random.default_rng(seed).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)
    w[0], w[1] = 0, 0xFFFFFFFF
    w[2] = [0, 0xFFFFFFFF] * 4
    return w


@pytest.mark.parametrize("n", [8, 9, 64, 4096])
def test_draw_is_the_kth_of_the_remaining(n):
    w = words_for(n, 200)
    s = tf.draw(w, n)
    assert s.dtype == np.int32 and s.shape == (200, 8)
    assert np.array_equal(s, brute(w, n))
    assert s.min() >= 0 and s.max() < n
    assert all(len(set(row.tolist())) == 8 for row in s)
    if n == 8:
        assert all(sorted(row.tolist()) == list(range(8)) for row in s)
    assert s[0].tolist() == list(range(8))  # the word 0 takes the first index left, every time
    # 0xFFFFFFFF % (n - k), as the k-th of the remaining
    assert s[1].tolist() == brute(w[1:2], n)[0].tolist()


# ---- trackframe_plan.h behind a ctypes shim
SRC = r'''
#include "trackframe_plan.h"
extern "C" const char *tfp_check(const int *iv, const double *dv, int have_image, int cam_model, int have_words, int table_count) {
  static const unsigned char px = 0;
  static const unsigned words[8] = {0};
  LfvioCamera cam = {};
  cam.model = cam_model, cam.c = 1.0;
  LfvioTrackFrameIn in = {};
  in.width = iv[0], in.height = iv[1], in.publish = iv[2], in.win_size = iv[3], in.max_level = iv[4], in.max_iterations = iv[5];
  in.border = iv[6], in.max_count = iv[7], in.min_distance = iv[8], in.mask_radius = iv[9], in.num_samples = iv[10], in.capacity = iv[11];
  in.time = dv[0], in.epsilon = dv[1], in.min_eig_threshold = dv[2], in.quality_level = dv[3];
  in.image = have_image ? &px : nullptr, in.camera = cam_model >= 0 ? &cam : nullptr, in.sample_words = have_words ? words : nullptr;
  return trackframe_check(&in, table_count);
}
extern "C" void tfp_draw(const unsigned *words, int n, int *out) { trackframe_draw(words, n, out); }
extern "C" int tfp_bound(int table_count, int max_count, int publish) { return trackframe_bound(table_count, max_count, publish != 0); }
extern "C" int tfp_sizes(int *out) {
  const int v[] = {(int)sizeof(LfvioTrackFrameIn), (int)sizeof(LfvioTrackFrameOut), (int)sizeof(LfvioTrackFrameStages)};
  for (unsigned k = 0; k < 3; k++) out[k] = v[k];
  return 3;
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="trackframe_plan_")
    src, so = os.path.join(d, "tfp.cpp"), os.path.join(d, "libtfp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.tfp_check.restype = C.c_char_p
    so.tfp_check.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)] + [C.c_int] * 4
    so.tfp_draw.restype = None
    so.tfp_draw.argtypes = [C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int)]
    return so


def test_header_draw_equals_the_restatement(lib):
    for n in (8, 9, 64, 4096):
        w = words_for(100 + n, 50)
        want = tf.draw(w, n)
        got = np.zeros(8, np.int32)
        for s in range(len(w)):
            row = np.ascontiguousarray(w[s])
            lib.tfp_draw(row.ctypes.data_as(C.POINTER(C.c_uint)), n, got.ctypes.data_as(C.POINTER(C.c_int)))
            assert got.tolist() == want[s].tolist(), (n, s)


GOOD = dict(tf.DEFAULTS, width=161, height=123, num_samples=100, capacity=150)
INT_KEYS = ("width", "height", "publish", "win_size", "max_level", "max_iterations", "border", "max_count", "min_distance", "mask_radius", "num_samples",
            "capacity")


def plan_says(lib, p, table_count=0, have_image=True, cam_model=0, have_words=True, publish=True, time=1.0):
    q = dict(p, publish=int(publish))
    iv = (C.c_int * 12)(*[int(q[k]) for k in INT_KEYS])
    dv = (C.c_double * 4)(time, p["epsilon"], p["min_eig_threshold"], p["quality_level"])
    return lib.tfp_check(iv, dv, int(have_image), cam_model, int(have_words), table_count)


def test_plan_header_equals_the_restatements_checks(lib):
    nan, inf = float("nan"), float("inf")
    values = dict(
        width=(15, 16, 8192, 8193, -1), height=(15, 16, 8192, 8193), win_size=(3, 4, 5, 21, 40, 41, 43), max_level=(-1, 0, 5, 6),
        max_iterations=(0, 1, 100, 101), epsilon=(0.0, -1.0, 1e-9, nan), min_eig_threshold=(-1e-9, 0.0, nan), border=(-1, 0, 1000),
        max_count=(0, 1, 150, 151, 4096, 4097), quality_level=(0.0, 1e-6, 1.0, 1.0001, nan), min_distance=(-1, 0, 1024, 1025),
        mask_radius=(-1, 0, 1024, 1025), num_samples=(0, 1, 1024, 1025, -5), capacity=(149, 150, 4096, 4097, 0))
    total = refused = 0
    for key, vs in values.items():
        for v in vs:
            p = dict(GOOD, **{key: v})
            why, want = plan_says(lib, p), tf.check(p, 0)
            assert (why is not None) == want, (key, v, why)
            assert why is None or why.startswith(b"lfvio_"), why
            total, refused = total + 1, refused + want
    assert 20 < refused < total
    assert plan_says(lib, GOOD) is None and not tf.check(GOOD, 0)
    # the table's count beside the capacity
    for count, cap in ((150, 150), (151, 150), (200, 200), (4096, 4096), (200, 199)):
        p = dict(GOOD, capacity=cap)
        assert (plan_says(lib, p, table_count=count) is not None) == tf.check(p, count) == (cap < max(150, count)), (count, cap)
    # pointers, the camera, the time
    assert plan_says(lib, GOOD, have_image=False) is not None and tf.check(GOOD, 0, have_image=False)
    assert plan_says(lib, GOOD, cam_model=-1) is not None and tf.check(GOOD, 0, cam=None)
    assert plan_says(lib, GOOD, cam_model=1) is not None and tf.check(GOOD, 0, cam=dict(tr.PAL, model=1))
    assert plan_says(lib, GOOD, have_words=False) is not None and tf.check(GOOD, 0, have_words=False)
    assert plan_says(lib, GOOD, have_words=False, publish=False) is None and not tf.check(GOOD, 0, have_words=False, publish=False)
    for t in (nan, inf, -inf, 0.0, -5.0, 1e300):
        assert (plan_says(lib, GOOD, time=t) is not None) == tf.check(GOOD, 0, time=t) == bool(np.isnan(t)), t
    for count, mc, pub in ((0, 40, True), (60, 40, True), (60, 40, False), (0, 40, False)):
        assert lib.tfp_bound(count, mc, int(pub)) == (max(count, mc) if pub else count)


def test_struct_sizes(lib):
    from lfvio import abi

    v = (C.c_int * 3)()
    assert lib.tfp_sizes(v) == 3
    assert list(v) == [C.sizeof(abi.TrackFrameInC), C.sizeof(abi.TrackFrameOutC), C.sizeof(abi.TrackFrameStagesC)]


def test_restated_frames_keep_the_tables_invariants():
    """Three frames of 64 x 48 through the restatement: ids unique and numbered in order, counts grow by one, a corner's velocity is
    zero on its first two frames."""
    W, H = 64, 48
    f = klt_ref.texture(5)
    cam = dict(cx=32.0, cy=24.0, c=1.0, d=0.0, e=0.0, poly=tr.PAL["poly"])
    fr = tf.Frame()
    kw = dict(win_size=11, max_level=1, max_count=12, min_distance=6, mask_radius=6)
    first = {}
    for k in range(3):
        _, inv = klt_ref.warp(W, H, shift=(0.5 * k, -0.25 * k))
        r = fr.read(klt_ref.render(f, W, H, inv), 1.0 + 0.05 * k, cam, words=words_for(k, 20), **kw)
        ids = r["ids"].tolist()
        assert len(set(ids)) == len(ids) and min(ids) >= 0 and len(ids) <= 12
        for i, c, v in zip(ids, r["track_cnt"].tolist(), r["velocity_3d"]):
            first.setdefault(i, k)
            assert c == k - first[i] + 1 and v.any() == (k - first[i] >= 2), (k, i)
    assert fr.n_id == len(first) and len(r["ids"]) >= 6


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi
    from lfvio.engine import Engine

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("lfvio_track_frame", "lfvio_track_frame_reset"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    for name in ("track_frame", "track_frame_reset"):
        assert callable(getattr(Engine, name)), name
