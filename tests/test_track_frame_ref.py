"""CPU tests of lfvio_track_frame's specification (tests/track_frame_ref.py), its host-side checks (lf-vio_amd/csrc/trackframe_plan.h,
compiled alone with g++) and the ABI names.

  1  draw() against a brute-force "k-th of the remaining indices" restatement at n = 8, 9, 64 and 4096; at n = 8 every set is a
     permutation of 0 .. 7; the indices are distinct and in range; the words 0 and 0xFFFFFFFF
  2  trackframe_draw of the header gives draw()'s indices
  3  trackframe_plan.h refuses what track_frame_ref.check refuses, field by field
  4  a frame of the restatement on a small image: the table's invariants
  5  the two names are in the header, in abi.HIP_SYMBOLS and in the built library
  6  behind the copy down (both frame routes): trackframe_counts_check accepts every count at its bound and refuses each one beyond
     it or negative; trackframe_out_check wants every array; track_reject_copy leaves E without a model; trackframe_emit changes
     exactly the first num_points entries and num_rows rows of outputs prefilled with a pattern"""
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
extern "C" int tfp_dev_bytes() { return (int)sizeof(TfDev); }
extern "C" int tfp_counts_check(const TfDev *v, int table_count, int max_count, int publish, int num_rows) {
  return trackframe_counts_check(*v, table_count, max_count, publish != 0, num_rows);
}
extern "C" int tfp_out_check(const LfvioTrackFrameOut *out, const LfvioTrackMessage *msg) { return trackframe_out_check(out, msg); }
extern "C" void tfp_reject_copy(LfvioTrackRejectOut *dst, const LfvioTrackRejectOut *src) { track_reject_copy(dst, *src); }
// seg: a down segment; at: the offsets of [TfDev, table, un, un3d, vel, msg] in it (msg < 0: no rows came down)
extern "C" void tfp_emit(const char *seg, const long long *at, long long B, int levels_used, int publish, LfvioTrackFrameOut *out, LfvioTrackMessage *msg) {
  const TfDown d = {(const TfDev *)(seg + at[0]), seg + at[1], (size_t)B, seg + at[2], seg + at[3], seg + at[4], at[5] < 0 ? nullptr : seg + at[5]};
  trackframe_emit(d, levels_used, publish != 0, out, msg);
}
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
    so.tfp_counts_check.argtypes = [C.c_void_p] + [C.c_int] * 4
    so.tfp_out_check.argtypes = [C.c_void_p, C.c_void_p]
    so.tfp_reject_copy.restype = so.tfp_emit.restype = None
    so.tfp_reject_copy.argtypes = [C.c_void_p, C.c_void_p]
    so.tfp_emit.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
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


# ---- behind the copy down: the counts against their bounds, then the caller's arrays from a down segment
def dev_of(abi, n1=0, n2=0, num_points=0, num_new=0, num_kept=0, num_corners=0, status=0):
    class TfDevC(C.Structure):
        _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("num_points", C.c_int), ("num_new", C.c_int), ("reject", abi.TrackRejectOutC), ("detect", abi.GftOutC)]

    v = TfDevC(n1, n2, num_points, num_new)
    v.reject.status, v.reject.best_sample, v.reject.num_inliers, v.reject.best_score = status, 17, 23, 0.625
    v.reject.E[:] = [0.5 + k for k in range(9)]
    v.detect.num_kept, v.detect.num_corners, v.detect.num_candidates, v.detect.max_response = num_kept, num_corners, 999, 12.5
    return v


def test_counts_check_accepts_the_bounds_and_refuses_one_beyond(lib):
    from lfvio import abi

    assert lib.tfp_dev_bytes() == 136 == C.sizeof(dev_of(abi))
    N0, MC = 60, 40
    for pub in (0, 1):
        for table_count, max_count in ((N0, MC), (MC, N0), (0, 1), (4096, 4096)):
            B = max(table_count, max_count) if pub else table_count
            at_bound = dict(num_points=B, n1=table_count, num_kept=table_count, num_corners=max_count)
            ok = lambda num_rows=None, **kw: lib.tfp_counts_check(C.byref(dev_of(abi, **dict(at_bound, **kw))), table_count, max_count, pub,
                                                                  B if num_rows is None else num_rows)
            assert ok() == 1 and ok(num_points=0, n1=0, num_kept=0, num_corners=0, num_rows=0) == 1  # each at its bound; all zero
            assert ok(n2=10 ** 9, num_new=-5) == 1  # (n2 and num_new size nothing on the host)
            # one count off at a time: one beyond its bound, or negative
            assert ok(num_points=B + 1) == 0 and ok(num_points=-1, num_rows=0) == 0
            assert ok(n1=table_count + 1) == 0 and ok(n1=-1) == 0
            assert ok(num_rows=B + 1) == 0 and ok(num_rows=-1) == 0 and (B == 0 or ok(num_points=B - 1, num_rows=B) == 0)  # rows <= points
            for key, bound in (("num_kept", table_count), ("num_corners", max_count)):  # the detector's: written only with publish
                assert ok(**{key: bound + 1}) == 1 - pub and ok(**{key: -1}) == 1 - pub


def test_out_check_wants_every_array(lib):
    from lfvio import abi

    f, i = (C.c_float * 4)(), (C.c_int * 4)()
    names = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")

    def out(missing=None):
        o = abi.TrackFrameOutC()
        for k in names:
            if k != missing:
                setattr(o, k, i if k in ("ids", "track_cnt") else f)
        return o

    rows, none = abi.TrackMessageC(0, f), abi.TrackMessageC()
    assert lib.tfp_out_check(C.byref(out()), None) == 1 and lib.tfp_out_check(C.byref(out()), C.byref(rows)) == 1
    assert lib.tfp_out_check(C.byref(out()), C.byref(none)) == 0
    for k in names:
        assert lib.tfp_out_check(C.byref(out(k)), None) == 0 and lib.tfp_out_check(C.byref(out(k)), C.byref(rows)) == 0, k


def test_reject_copy_leaves_e_without_a_model(lib):
    from lfvio import abi

    for status in (0, 1, 2):
        src, dst = dev_of(abi, status=status).reject, abi.TrackRejectOutC(9, 9, 9, 9.0)
        dst.E[:] = [-1.0] * 9
        lib.tfp_reject_copy(C.byref(dst), C.byref(src))
        assert (dst.status, dst.best_sample, dst.num_inliers, dst.best_score) == (status, 17, 23, 0.625)
        assert list(dst.E) == (list(src.E) if status == 0 else [-1.0] * 9)


PATTERN = 0xA5


@pytest.mark.parametrize("B", [1, 150, 4096])
def test_emit_writes_exactly_the_counted_entries(lib, B):
    """A down segment laid out as the routes lay it (256-aligned segments of B entries), outputs of exactly B entries prefilled with
    a pattern: after trackframe_emit the first num_points entries (num_rows rows) are the segment's, every byte behind them is the
    pattern still, and the scalars are the TfDev's — the rejection's and the detector's records only with publish."""
    from lfvio import abi

    rng = np.random.default_rng(B)
    sizes = [136, B * 16, B * 8, B * 12, B * 12, 16 + B * 36]
    at, end = [], 0
    for s in sizes:
        at.append(end)
        end = (end + s + 255) // 256 * 256
    for n in sorted({0, 1, B}):
        for publish, with_msg, status in ((1, 1, 0), (1, 1, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            seg = rng.integers(0, 160, end, dtype=np.uint8)  # (never the pattern)
            num_rows = n if n < 2 else n - 1
            dev = dev_of(abi, n1=n, n2=max(n - 1, 0), num_points=n, num_new=n // 2, num_kept=n // 3, num_corners=n // 2, status=status)
            seg[at[0]:at[0] + 136] = np.frombuffer(bytes(dev), np.uint8)
            seg[at[5]:at[5] + 4] = np.frombuffer(np.int32(num_rows).tobytes(), np.uint8)
            rows_came = bool(publish and with_msg)
            offs = (C.c_longlong * 6)(*(at[:5] + [at[5] if rows_came else -1]))
            per = dict(pts=8, ids=4, track_cnt=4, un_pts=8, un_pts_3d=12, velocity_3d=12)
            arrays = {k: np.full(B * v, PATTERN, np.uint8) for k, v in per.items()}
            rows = np.full(B * 36, PATTERN, np.uint8)
            out = abi.TrackFrameOutC(-7, -7, -7, -7, -7)
            C.memset(C.byref(out.reject), PATTERN, C.sizeof(out.reject)), C.memset(C.byref(out.detect), PATTERN, C.sizeof(out.detect))
            for k, a in arrays.items():
                setattr(out, k, a.ctypes.data_as(C.POINTER(C.c_int if k in ("ids", "track_cnt") else C.c_float)))
            msg = abi.TrackMessageC(-7, rows.ctypes.data_as(C.POINTER(C.c_float)))
            lib.tfp_emit(seg.ctypes.data, offs, B, 3, publish, C.byref(out), C.byref(msg) if with_msg else None)
            case = (B, n, publish, with_msg, status)
            assert (out.num_points, out.num_new, out.levels_used, out.num_tracked, out.num_after_reject) == (n, n // 2, 3, n, max(n - 1, 0)), case
            r, d = out.reject, out.detect
            if publish:
                assert (r.status, r.best_sample, r.num_inliers, r.best_score) == (status, 17, 23, 0.625), case
                assert list(r.E) == (list(dev.reject.E) if status == 0 else [0.0] * 9), case  # no model: E is zero
                assert (d.num_kept, d.num_corners, d.num_candidates, d.max_response) == (n // 3, n // 2, 999, 12.5), case
            else:
                assert bytes(r) == bytes(C.sizeof(r)) and bytes(d) == bytes(C.sizeof(d)), case
            src = dict(pts=(at[1], 8), ids=(at[1] + B * 8, 4), track_cnt=(at[1] + B * 12, 4), un_pts=(at[2], 8), un_pts_3d=(at[3], 12), velocity_3d=(at[4], 12))
            for k, (o, size) in src.items():
                want = np.full(B * size, PATTERN, np.uint8)
                want[:n * size] = seg[o:o + n * size]
                assert np.array_equal(arrays[k], want), (case, k)
            want = np.full(B * 36, PATTERN, np.uint8)
            if rows_came:
                want[:num_rows * 36] = seg[at[5] + 16:at[5] + 16 + num_rows * 36]
            assert np.array_equal(rows, want), case
            assert msg.num_rows == ((num_rows if rows_came else 0) if with_msg else -7), case


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
