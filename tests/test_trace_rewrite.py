"""CPU tests of the recording walk (lf-vio_amd/host/trace_rewrite.{h,cpp}: rewriteRecordings, which trackRecording runs with n = 1 and
trackRecordings with n streams), compiled with g++ -ffp-contract=off -Wall -Werror behind a ctypes shim, with replay.cpp for
Trace::load and no device library on the link line.  The round is a stub that follows a plan: image k of a recording is dropped,
restarts, is tracked only or is published with two fabricated rows.  The recordings are lfvio.trace.make_image_stream's at scale 16
(80 x 60), of 4, 4 and 2 images.

  1  n = 1 and n = 3 (unequal lengths): every output equals the file built here in Python from the input — every record that is no
     image copied byte for byte in its place, a type-5 record with the stamp for a restart, a type-2 record with the packed 12-byte head
     and the rows for a publication, nothing otherwise — TrackStats is exact, the stub saw every image's head and pixels as the file has
     them, round r held the r-th image of every recording that still had one, and a recording alone gives what it gives among three
  2  a missing file, one cut in the middle of a record and n = 0 give -3; a round that returns a negative value gives -2 with that
     round's images already counted in raw_images
  3  writeBytes: the bytes, and -1 where the file cannot be made
  4  tests/tools/track_node_walk.cpp, a stand-alone program over the same header and walk, builds with -fsanitize=address,undefined and
     runs clean"""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lf-vio_amd", "host")
DROPPED, RESTART, TRACKED_ONLY, FIRST_SKIPPED, PUBLISHED = 0, 1, 2, 3, 4
ROUNDS, STATS = 8, ("raw_images", "dropped", "restarts", "tracked_only", "published", "rows", "tracker_ms")

SRC = r'''
#include "trace_rewrite.h"
using namespace lfvio;
#define API extern "C" __attribute__((visibility("default")))

// The stub round: image k of stream i becomes plan[i][k]; a publication has two rows, row r column c = 100 k + 9 r + c + width / 1024.
// seen[round][i][7] = {present, stamp, width, height, step, encoding, the sum of the first height * step bytes behind `pixels`}.
// Round number fail_round returns -1 without touching the entries.
API int tr_walk(int n, const char *const *paths, const int *plan, int fail_round, unsigned char *out, long cap, long *sizes, double *stats, double *seen) {
  std::vector<std::vector<char>> outs;
  std::vector<TrackStats> st((size_t)(n > 0 ? n : 1));
  std::vector<int> k((size_t)(n > 0 ? n : 1), 0);
  int round = 0;
  const int rc = rewriteRecordings(n, paths, &outs, st.data(), [&](BatchEntry *e) {
    if (round == fail_round) return -1;
    for (int i = 0; i < n; i++) {
      double *s = seen + ((size_t)round * n + i) * 7;
      s[0] = e[i].present;
      if (!e[i].present) continue;
      double sum = 0;
      for (long b = 0; b < (long)e[i].height * e[i].step; b++) sum += e[i].pixels[b];
      s[1] = e[i].stamp, s[2] = e[i].width, s[3] = e[i].height, s[4] = e[i].step, s[5] = e[i].encoding, s[6] = sum;
      e[i].result = plan[i * 8 + k[i]];
      if (e[i].result == TrackResults::PUBLISHED) {
        e[i].msg.t = e[i].stamp;
        e[i].msg.v.resize(18);
        for (int c = 0; c < 18; c++) e[i].msg.v[c] = (float)(100 * k[i] + c) + (float)e[i].width / 1024.0f;
      }
      k[i]++;
    }
    round++;
    return 0;
  });
  for (int i = 0; i < n; i++) {
    std::memcpy(stats + 7 * i, &st[i], sizeof st[i]);
    sizes[i] = i < (int)outs.size() ? (long)outs[i].size() : -1;
    if (sizes[i] > 0 && sizes[i] <= cap) std::memcpy(out + (size_t)i * cap, outs[i].data(), outs[i].size());
  }
  return rc;
}
API int tr_write(const char *path, const char *bytes, long n) { return writeBytes(path, std::vector<char>(bytes, bytes + n)); }
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="trace_rewrite_")
    src, so = os.path.join(d, "rewrite.cpp"), os.path.join(d, "librewrite.so")
    open(src, "w").write(SRC)
    # replay.cpp for Trace::load; its replay(), which drives the estimator, is not referenced and leaves with its section: -z defs makes
    # the link fail where anything that stays names a symbol of another library
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-fvisibility=hidden", "-ffunction-sections",
                           "-Wl,--gc-sections", "-Wl,-z,defs", "-I", HOST, src, os.path.join(HOST, "trace_rewrite.cpp"), os.path.join(HOST, "replay.cpp"), "-o", so])
    so = C.CDLL(so)
    so.tr_walk.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_double),
                           C.POINTER(C.c_double)]
    so.tr_write.argtypes = [C.c_char_p, C.c_char_p, C.c_long]
    return so


PLANS = ([DROPPED, PUBLISHED, RESTART, PUBLISHED], [DROPPED, TRACKED_ONLY, PUBLISHED, FIRST_SKIPPED], [DROPPED, PUBLISHED])


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """Three recordings of 4, 4 and 2 images with their bytes: made once, shared, never changed."""
    from lfvio import trace

    d = tmp_path_factory.mktemp("trace_rewrite")
    out = []
    for seed, plan in enumerate(PLANS):
        p = str(d / f"raw{seed}.lfvt")
        made = trace.make_image_stream(p, seed=seed, n_frames=len(plan), scale=16)
        assert (made["width"], made["height"]) == (80, 60)
        out.append((p, open(p, "rb").read()))
    return out


def records(body):
    """-> the 8-byte file head, [(type, payload)] in file order."""
    at, out = 8, []
    while at < len(body):
        typ, n = struct.unpack_from("<II", body, at)
        out.append((typ, body[at + 8:at + 8 + n]))
        at += 8 + n
    assert at == len(body)
    return body[:8], out


def expected(body, plan):
    """The rewritten file, its stats without tracker_ms, and the images' heads as the stub must see them."""
    head, recs = records(body)
    out, k, st, seen = [head], 0, dict.fromkeys(STATS[:6], 0.0), []
    for typ, pay in recs:
        if typ != 10:
            out.append(struct.pack("<II", typ, len(pay)) + pay)
            continue
        stamp, w, h, step, enc = struct.unpack_from("<dIIII", pay, 0)
        seen.append([1.0, stamp, w, h, step, enc, float(np.frombuffer(pay, np.uint8, h * step, 24).sum(dtype=np.float64))])
        what = plan[k]
        st["raw_images"] += 1
        if what == DROPPED:
            st["dropped"] += 1
        elif what == RESTART:
            st["restarts"] += 1
            out.append(struct.pack("<IId", 5, 8, stamp))
        elif what == PUBLISHED:
            rows = (np.arange(18, dtype=np.float32) + np.float32(100 * k)) + np.float32(w) / np.float32(1024.0)
            st["published"] += 1
            st["rows"] += 2
            out.append(struct.pack("<IIdI", 2, 12 + 72, stamp, 2) + rows.astype("<f4").tobytes())  # the packed head: f64 stamp, u32 n
        else:
            st["tracked_only"] += 1
        k += 1
    assert k == len(plan)
    return b"".join(out), st, seen


def walk(lib, paths, plans, fail_round=-1):
    n, cap = len(paths), 1 << 20
    arr = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
    plan = np.zeros((max(n, 1), 8), np.int32)
    for i, p in enumerate(plans):
        plan[i, :len(p)] = p
    out, sizes, stats, seen = np.zeros((max(n, 1), cap), np.uint8), (C.c_long * max(n, 1))(), np.full((max(n, 1), 7), -1.0), np.zeros((ROUNDS, max(n, 1), 7))
    rc = lib.tr_walk(n, arr, plan.ctypes.data_as(C.POINTER(C.c_int)), fail_round, out.ctypes.data, cap, sizes, stats.ctypes.data_as(C.POINTER(C.c_double)),
                     seen.ctypes.data_as(C.POINTER(C.c_double)))
    assert all(s <= cap for s in sizes)
    return rc, [out[i, :max(sizes[i], 0)].tobytes() for i in range(n)], [dict(zip(STATS, row.tolist())) for row in stats[:n]], seen


# ---- 1
def test_one_and_three(lib, recordings):
    paths, bodies = [p for p, _ in recordings], [b for _, b in recordings]
    want = [expected(b, plan) for b, plan in zip(bodies, PLANS)]
    for b, (w, _, _) in zip(bodies, want):  # the expectation is no copy of the input and no empty file
        types_in, types_out = [t for t, _ in records(b)[1]], [t for t, _ in records(w)[1]]
        assert 10 in types_in and 10 not in types_out and 2 in types_out and [t for t in types_in if t != 10] == [t for t in types_out if t not in (2, 5)]
    assert 5 in [t for t, _ in records(want[0][0])[1]]
    rc, outs, stats, seen = walk(lib, paths, PLANS)
    assert rc == 0
    for i in range(3):
        assert outs[i] == want[i][0], i
        assert {k: v for k, v in stats[i].items() if k != "tracker_ms"} == want[i][1], i
        assert stats[i]["tracker_ms"] >= 0.0
        # round r holds the r-th image of every recording that still has one
        for r in range(ROUNDS):
            assert seen[r, i].tolist() == (want[i][2][r] if r < len(PLANS[i]) else [0.0] * 7), (i, r)
    assert want[0][2][0][6] > 0  # pixels, not zeros
    # every recording alone: the same bytes and stats as among the three
    for i in range(3):
        rc1, out1, st1, seen1 = walk(lib, [paths[i]], [PLANS[i]])
        assert rc1 == 0 and out1[0] == outs[i], i
        assert {k: v for k, v in st1[0].items() if k != "tracker_ms"} == want[i][1], i
        assert seen1[:len(PLANS[i]), 0].tolist() == want[i][2]


# ---- 2
def test_refusals(lib, recordings, tmp_path):
    paths, bodies = [p for p, _ in recordings], [b for _, b in recordings]
    zero = dict.fromkeys(STATS, 0.0)
    rc, _, stats, _ = walk(lib, [paths[0], str(tmp_path / "missing.lfvt"), paths[2]], PLANS)
    assert rc == -3 and stats == [zero] * 3
    # cut in the middle of a record: in the last image's head and in its pixels
    _, recs = records(bodies[1])
    at, cuts = 8, []
    for typ, pay in recs:
        if typ == 10:
            cuts = [at + 8 + 12, at + 8 + 24 + len(pay) // 2]  # (the last image's)
        at += 8 + len(pay)
    for cut in cuts:
        short = str(tmp_path / f"cut{cut}.lfvt")
        open(short, "wb").write(bodies[1][:cut])
        rc, _, stats, _ = walk(lib, [short], [PLANS[1]])
        assert rc == -3 and stats[0]["published"] == 0, cut
        assert walk(lib, [paths[0], short], PLANS[:2])[0] == -3
    assert walk(lib, [], [])[0] == -3
    # a round that fails: -2, its images counted
    for fail_round, counted in ((0, [1, 1, 1]), (2, [3, 3, 2]), (3, [4, 4, 2])):
        rc, _, stats, seen = walk(lib, paths, PLANS, fail_round=fail_round)
        assert rc == -2 and [s["raw_images"] for s in stats] == counted, fail_round
        assert not seen[fail_round:].any()
        done = [expected_prefix(PLANS[i], min(fail_round, len(PLANS[i]))) for i in range(3)]
        assert [(s["dropped"], s["restarts"], s["tracked_only"], s["published"]) for s in stats] == done, fail_round
    rc, _, stats, _ = walk(lib, [paths[1]], [PLANS[1]], fail_round=0)  # as a tracker whose constructor failed: at its first image
    assert rc == -2 and stats[0]["raw_images"] == 1 and stats[0]["dropped"] == 0


def expected_prefix(plan, k):
    p = plan[:k]
    return (float(p.count(DROPPED)), float(p.count(RESTART)), float(p.count(TRACKED_ONLY) + p.count(FIRST_SKIPPED)), float(p.count(PUBLISHED)))


# ---- 3
def test_write_bytes(lib, tmp_path):
    body = bytes(range(256)) * 5
    p = str(tmp_path / "w.bin")
    assert lib.tr_write(p.encode(), body, len(body)) == 0 and open(p, "rb").read() == body
    assert lib.tr_write(p.encode(), b"", 0) == 0 and open(p, "rb").read() == b""  # an empty vector truncates
    assert lib.tr_write(str(tmp_path / "no_such_dir" / "w.bin").encode(), body, len(body)) == -1


# ---- 4
def test_walk_under_the_sanitizers(recordings):
    d = tempfile.mkdtemp(prefix="track_node_walk_")
    exe = os.path.join(d, "track_node_walk")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffunction-sections", "-Wl,--gc-sections", "-I", HOST, os.path.join(ROOT, "tests", "tools", "track_node_walk.cpp"),
                           os.path.join(HOST, "trace_rewrite.cpp"), os.path.join(HOST, "replay.cpp"), "-o", exe])
    r = subprocess.run([exe] + [p for p, _ in recordings], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "0 wrong" in r.stdout, r.stdout + r.stderr
