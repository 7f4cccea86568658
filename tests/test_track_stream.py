"""CPU test of the tracker's stream state (lf-vio_amd/csrc/track_stream.h: the scalars of one image stream and the moves the host
makes on them).  The header is plain C++, compiled here alone with g++ -Wall -Werror into a small shared object and driven through
ctypes, like tests/test_call_state.py.  `Restated` below is a few lines of Python per move that restate what the host code did
before the header existed — field by field, for the single route's four states and for the batched route's slot, which were the
same thirteen ints and one double under different names.

Asserted: every move of the header gives the restatement's struct — frame commits with num_points 0 and > 0, a size change, fewer
levels then more, the three resets (each leaves what the others own, and all leave the base mask), the mask-fit rule; and a sequence
of calls driven the way the single route drives it and the way the batched route drives a slot ends in equal structs."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = "pcur w h built valid mw mh mask_set tcur count n_id mcur mcount".split()
SRC = r'''
#include "track_stream.h"
extern "C" int ts_move(int *v, double *time, int move, const int *a, double t) {
  TrackStream s;
  s.pcur = v[0], s.w = v[1], s.h = v[2], s.built = v[3], s.valid = v[4] != 0, s.mw = v[5], s.mh = v[6], s.mask_set = v[7] != 0;
  s.tcur = v[8], s.count = v[9], s.n_id = v[10], s.mcur = v[11], s.mcount = v[12], s.time = *time;
  int r = 0;
  switch (move) {
    case 0: r = s.resident(a[0], a[1]); break;
    case 1: r = s.prev_built(a[0], a[1], a[2]); break;
    case 2: r = s.levels_missing(a[0], a[1], a[2]); break;
    case 3: s.resident_built(a[0]); break;
    case 4: r = s.resident_w(); break;
    case 5: r = s.mask_fits(a[0], a[1]); break;
    case 6: s.mask_is(a[0], a[1]); break;
    case 7: s.mask_cleared(); break;
    case 8: s.commit_flow(a[0], a[1], a[2]); break;
    case 9: s.commit_undistort(a[0], t); break;
    case 10: s.commit_frame(a[0], a[1], a[2], a[3], a[4], t); break;
    case 11: s.reset_flow(); break;
    case 12: s.reset_map(); break;
    case 13: s.reset_frame(); break;
    default: r = -1;
  }
  const int w[13] = {s.pcur, s.w, s.h, s.built, s.valid, s.mw, s.mh, s.mask_set, s.tcur, s.count, s.n_id, s.mcur, s.mcount};
  for (int k = 0; k < 13; k++) v[k] = w[k];
  *time = s.time;
  return r;
}
extern "C" int ts_fresh(int *v, double *time) {
  TrackStream s;
  const int w[13] = {s.pcur, s.w, s.h, s.built, s.valid, s.mw, s.mh, s.mask_set, s.tcur, s.count, s.n_id, s.mcur, s.mcount};
  for (int k = 0; k < 13; k++) v[k] = w[k];
  *time = s.time;
  return (int)sizeof(TrackStream);
}
'''
MOVES = ("resident prev_built levels_missing resident_built resident_w mask_fits mask_is mask_cleared commit_flow commit_undistort "
         "commit_frame reset_flow reset_map reset_frame").split()


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="track_stream_")
    src, so = os.path.join(d, "ts.cpp"), os.path.join(d, "libts.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.ts_move.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_double]
    so.ts_fresh.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    return so


class Header:
    """a TrackStream of the header, held as its fields between the moves"""

    def __init__(self, lib):
        self.lib, self.v, self.t = lib, (C.c_int * 13)(), C.c_double(0.0)
        lib.ts_fresh(self.v, C.byref(self.t))

    def move(self, what, *a, t=0.0):
        args = (C.c_int * 5)(*(list(a) + [0] * (5 - len(a))))
        return self.lib.ts_move(self.v, C.byref(self.t), MOVES.index(what), args, t)

    def state(self):
        return dict(zip(FIELDS, list(self.v)), time=self.t.value)


class Restated:
    """The host code before track_stream.h.  The single route kept klt = (cur, w, h, built, valid), gft = (mw, mh, mask_set),
    tframe = (cur, count, n_id) and track = (cur, count, time); a slot of the batched route kept the same under the names below."""

    def __init__(self):
        self.s = dict(pcur=0, w=0, h=0, built=0, valid=0, mw=0, mh=0, mask_set=0, tcur=0, count=0, n_id=0, mcur=0, mcount=0, time=0.0)

    def state(self):
        return dict(self.s)

    def same(self, W, H):  # klt_pyramid's and the descriptor fill's `same`
        s = self.s
        return bool(s["valid"] and s["w"] == W and s["h"] == H)

    def resident(self, W, H):
        return int(self.same(W, H))

    def prev_built(self, W, H, LU):  # t.prev_built = same ? s.built : LU
        return self.s["built"] if self.same(W, H) else LU

    def levels_missing(self, W, H, LU):  # if (same && k.built < LU) klt_build(.., k.built, LU)
        return LU - self.s["built"] if self.same(W, H) and self.s["built"] < LU else 0

    def resident_built(self, LU):  # k.built = LU
        self.s["built"] = LU

    def resident_w(self):  # c->klt.valid ? c->klt.w : 0
        return self.s["w"] if self.s["valid"] else 0

    def mask_fits(self, W, H):  # !(g.mask_set && (g.mw != W || g.mh != H))
        s = self.s
        return int(not (s["mask_set"] and (s["mw"] != W or s["mh"] != H)))

    def mask_is(self, W, H):  # g.mw = width, g.mh = height, g.mask_set = true
        self.s.update(mw=W, mh=H, mask_set=1)

    def mask_cleared(self):
        self.s["mask_set"] = 0

    def commit_flow(self, W, H, LU):  # klt_commit
        s = self.s
        s.update(pcur=1 - s["pcur"], w=W, h=H, built=LU, valid=1)

    def commit_undistort(self, N, t=0.0):  # lfvio_track_undistort: the N = 0 branch, and its last line
        s = self.s
        if N == 0:
            s.update(mcount=0, time=t)
        else:
            s.update(mcur=1 - s["mcur"], mcount=N, time=t)

    def commit_frame(self, W, H, LU, n, num_new, t=0.0):  # the last four lines of track_frame_run / of lfvio_track_batch_frame
        s = self.s
        s.update(pcur=1 - s["pcur"], w=W, h=H, built=LU, valid=1)
        if n:
            s["mcur"] = 1 - s["mcur"]
        s.update(mcount=n, time=t)
        s.update(tcur=1 - s["tcur"], count=n, n_id=s["n_id"] + num_new)

    def reset_flow(self):  # lfvio_klt_reset
        self.s["valid"] = 0

    def reset_map(self):  # lfvio_track_reset
        self.s.update(mcount=0, time=0.0)

    def reset_frame(self):  # lfvio_track_frame_reset, lfvio_track_batch_reset
        self.s.update(valid=0, mcount=0, time=0.0, count=0, n_id=0)


class Both:
    """every move through the header and the restatement, compared at once"""

    def __init__(self, lib):
        self.h, self.r = Header(lib), Restated()

    def __getattr__(self, what):
        def go(*a, t=None):
            kw = {} if t is None else dict(t=t)
            got, want = self.h.move(what, *a, **kw), getattr(self.r, what)(*a, **kw)
            assert self.h.state() == self.r.state(), (what, a, self.h.state(), self.r.state())
            if want is not None:
                assert got == want, (what, a, got, want)
            return got
        return go

    def state(self):
        return self.h.state()


def test_a_fresh_stream_is_all_zero(lib):
    h = Header(lib)
    assert h.state() == Restated().state()
    assert h.move("resident", 0, 0) == 0 and h.move("mask_fits", 161, 123) == 1 and h.move("resident_w") == 0


def test_frame_commits_with_and_without_points(lib):
    b = Both(lib)
    b.commit_frame(161, 123, 3, 0, 0, t=1.0)  # an empty first frame: the map does not swap
    assert b.state() == dict(Restated().state(), pcur=1, w=161, h=123, built=3, valid=1, tcur=1, time=1.0)
    b.commit_frame(161, 123, 3, 40, 40, t=1.05)
    s = b.state()
    assert (s["pcur"], s["tcur"], s["mcur"], s["count"], s["mcount"], s["n_id"], s["time"]) == (0, 0, 1, 40, 40, 40, 1.05)
    b.commit_frame(161, 123, 3, 37, 5, t=1.1)
    s = b.state()
    assert (s["pcur"], s["tcur"], s["mcur"], s["count"], s["mcount"], s["n_id"]) == (1, 1, 0, 37, 37, 45)
    b.commit_frame(161, 123, 3, 0, 0, t=1.15)  # every track lost: table and pyramid swap, the map stays where it is
    s = b.state()
    assert (s["pcur"], s["tcur"], s["mcur"], s["count"], s["mcount"], s["n_id"], s["time"]) == (0, 0, 0, 0, 0, 45, 1.15)


def test_size_change_and_levels(lib):
    b = Both(lib)
    assert b.resident(161, 123) == 0 and b.prev_built(161, 123, 3) == 3 and b.levels_missing(161, 123, 3) == 0
    b.commit_flow(161, 123, 3)
    assert b.resident(161, 123) == 1 and b.resident(123, 161) == 0 and b.resident(161, 124) == 0 and b.resident_w() == 161
    # another size: the new image is both images, nothing to build on the resident one
    assert b.prev_built(320, 240, 2) == 2 and b.levels_missing(320, 240, 5) == 0
    b.commit_flow(320, 240, 1)  # fewer levels ...
    assert b.state()["built"] == 1 and b.levels_missing(320, 240, 1) == 0 and b.levels_missing(320, 240, 0) == 0
    assert b.levels_missing(320, 240, 4) == 3 and b.prev_built(320, 240, 4) == 1  # ... then more: levels 2 .. 4 are to build
    b.resident_built(4)
    assert b.levels_missing(320, 240, 4) == 0 and b.prev_built(320, 240, 4) == 4
    b.commit_flow(320, 240, 4)
    assert b.prev_built(320, 240, 2) == 4 and b.levels_missing(320, 240, 2) == 0
    b.reset_flow()
    assert b.resident(320, 240) == 0 and b.resident_w() == 0 and b.levels_missing(320, 240, 5) == 0 and b.prev_built(320, 240, 5) == 5


def test_undistort_commits(lib):
    b = Both(lib)
    b.commit_undistort(12, t=2.0)
    assert (b.state()["mcur"], b.state()["mcount"], b.state()["time"]) == (1, 12, 2.0)
    b.commit_undistort(0, t=2.5)  # an empty map: no swap, the time moves on
    assert (b.state()["mcur"], b.state()["mcount"], b.state()["time"]) == (1, 0, 2.5)
    b.commit_undistort(4096, t=3.0)
    assert (b.state()["mcur"], b.state()["mcount"], b.state()["time"]) == (0, 4096, 3.0)


def busy(lib):
    b = Both(lib)
    b.mask_is(161, 123)
    b.commit_frame(161, 123, 3, 40, 40, t=1.0)
    b.commit_frame(161, 123, 3, 38, 2, t=1.1)
    b.commit_frame(161, 123, 3, 39, 3, t=1.2)
    return b


def test_each_reset_leaves_what_the_others_own(lib):
    b = busy(lib)
    before = b.state()
    b.reset_flow()
    assert b.state() == dict(before, valid=0)
    b = busy(lib)
    b.reset_map()
    assert b.state() == dict(before, mcount=0, time=0.0)
    b = busy(lib)
    b.reset_frame()
    assert b.state() == dict(before, valid=0, mcount=0, time=0.0, count=0, n_id=0)
    # the mask and every buffer index survive all three; a frame after the reset starts numbering at 0
    assert b.mask_fits(161, 123) == 1 and b.mask_fits(160, 123) == 0
    b.commit_frame(161, 123, 3, 7, 7, t=5.0)
    assert b.state()["n_id"] == 7 and b.state()["pcur"] == 1 - before["pcur"]


def test_the_mask_fit_rule(lib):
    b = Both(lib)
    assert b.mask_fits(161, 123) == 1 and b.mask_fits(16, 8192) == 1  # none set: every image fits
    b.mask_is(161, 123)
    assert b.mask_fits(161, 123) == 1 and b.mask_fits(123, 161) == 0 and b.mask_fits(161, 122) == 0 and b.mask_fits(162, 123) == 0
    b.mask_cleared()
    assert b.mask_fits(123, 161) == 1 and (b.state()["mw"], b.state()["mh"]) == (161, 123)
    b.mask_is(64, 48)
    assert b.mask_fits(64, 48) == 1 and b.mask_fits(161, 123) == 0


def test_single_and_slot_end_in_equal_structs(lib):
    """The same calls the way the single route drives its stream (klt_pyramid builds the missing levels and says so, then the commit)
    and the way the batched route drives a slot (the descriptor carries prev_built, the resident levels are built by a second pass
    of the launch loop and never recorded: the commit overwrites `built`)."""
    single, slot = Both(lib), Both(lib)
    calls = [(161, 123, 3, 0, 0, 1.0), (161, 123, 3, 40, 40, 1.05), (161, 123, 1, 38, 2, 1.1), (161, 123, 4, 0, 0, 1.15), (320, 240, 2, 25, 25, 1.2),
             (320, 240, 5, 25, 0, 1.25), "reset", (320, 240, 5, 9, 9, 7.0), "mask", (161, 123, 3, 9, 0, 7.1)]
    for call in calls:
        if call == "reset":
            single.reset_frame(), slot.reset_frame()
        elif call == "mask":
            single.mask_is(161, 123), slot.mask_is(161, 123)
        else:
            W, H, LU, n, new, t = call
            assert single.mask_fits(W, H) == slot.mask_fits(W, H) == 1
            if single.levels_missing(W, H, LU):
                single.resident_built(LU)
            assert slot.prev_built(W, H, LU) + slot.levels_missing(W, H, LU) == max(slot.prev_built(W, H, LU), LU)
            single.commit_frame(W, H, LU, n, new, t=t), slot.commit_frame(W, H, LU, n, new, t=t)
        assert single.state() == slot.state(), call
    assert single.state()["n_id"] == 9 and single.state()["count"] == 9  # (numbered from 0 again behind the reset)
