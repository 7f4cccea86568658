"""CPU tests of lfvio_track_reject / lfvio_track_undistort's restatement (tests/track_ref.py), its fixture
(tests/golden/track_cases.npz), the host-side checks (lf-vio_amd/csrc/track_plan.h, compiled alone with g++) and the ABI names.

  1  the restatement reproduces its fixture bit for bit
  2  track_ref.lift with c, d, e = 1, 0, 0 agrees with synth.ocam_lift_projective to 1e-12 |P|: two restatements that sum the
     polynomial in different orders (five terms, a few roundings each: ~1e-15), so the bound is loose by three orders on purpose
  3  every fixture case with a model meets conditions C1 and C2 of tests/test_two_view.py on the restatement, so that the cap of the
     device's mask comparison (tests/test_track.py) cannot hide a device error
  4  track_plan.h refuses what the restatement's checks refuse, field by field, and forms inv_scale as the restatement does
  5  the three names are in the header, in abi.HIP_SYMBOLS and in the built library"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import track_ref as tr
from golden import gen_track
from lfvio import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "track_cases.npz"))
    return {k: z[k] for k in z.files}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiub" else a


def test_restatement_reproduces_its_fixture(fx):
    rec = gen_track.build()
    assert sorted(rec) == sorted(fx)
    for k in rec:
        a, b = np.asarray(rec[k]), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)), k
    assert list(fx["names"]) == list(tr.CASES)
    assert sum(len(fx[f"{n}/cur"]) for n in tr.CASES) < 500  # a small file


def test_fixture_covers_what_it_should(fx):
    """Both cameras, the pixel on the centre (phi = 0), both signs of z, all three status values, gross outliers to reject."""
    st = {n: int(fx[f"{n}/status"]) for n in tr.CASES}
    assert set(st.values()) == {0, 1, 2}
    b = fx["skew_centre_45/bearing_cur"]
    assert np.array_equal(b[0], [0.0, 0.0, 1.0]) and tuple(fx["skew_centre_45/cam"][3:6]) != (1.0, 0.0, 0.0)
    for n in tr.CASES:
        if st[n] == 0:
            z = fx[f"{n}/bearing_cur"][:, 2]
            assert (z > 0).any() and (z < 0).any(), n
            m = fx[f"{n}/mask"]
            assert 8 <= m.sum() < len(m), n  # something is rejected
    for s in fx["sequences"]:
        ids = [fx[f"{s}/{j}/ids"] for j in range(int(fx[f"{s}/calls"]))]
        assert any((i == -1).any() for i in ids) and any(len(set(i.tolist())) < len(i) for i in ids)
        v = [fx[f"{s}/{j}/velocity_3d"] for j in range(len(ids))]
        assert not v[0].any() and all(x.any() for x in v[1:])


def test_lift_agrees_with_synth():
    rng = np.random.default_rng(5)
    px = rng.uniform([0.0, 0.0], [synth.OCAM_W, synth.OCAM_H], (4000, 2)).astype(np.float32)
    a, b = tr.lift(tr.PAL, px), synth.ocam_lift_projective(px.astype(np.float64))
    err = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    print("lift against synth: worst", err.max())
    assert err.max() <= 1e-12
    n = tr.norm(a)
    assert np.allclose(np.linalg.norm(tr.bearings(tr.PAL, px), axis=1), 1.0, rtol=0, atol=4e-16) and np.all(n > 0)
    # the affine part: projecting a ray and lifting the pixel gives the ray back (synth's pair is consistent to 0.011 deg)
    rays = synth.ocam_lift_projective(px.astype(np.float64))
    back = tr.bearings(tr.SKEW, tr.project(tr.SKEW, rays).astype(np.float32))
    ang = np.degrees(np.arccos(np.clip(np.sum(back * rays / np.linalg.norm(rays, axis=1, keepdims=True), axis=1), -1, 1)))
    inside = np.degrees(np.arccos(rays[:, 2] / np.linalg.norm(rays, axis=1)))
    assert ang[(inside > 40) & (inside < 120)].max() < 0.05


def test_fixture_cases_meet_c1_c2():
    n = 0
    for name in tr.CASES:
        cam, cur, forw, samples = tr.make_case(name)
        r = tr.reject(cam, cur, forw, samples)
        if r["status"] == 0:
            assert tr.conditions(r), (name, r["c1_gap"], r["c2_margin"])
            n += 1
    assert n >= 4


def test_undistort_map_semantics():
    """insert-once, ids as passed, -1 never looked up, the empty map, dt = 0."""
    cam, u = tr.PAL, tr.Undistort()
    p = np.array([[300.0, 200.0], [800.0, 700.0], [500.0, 100.0]], np.float32)
    r0 = u(cam, p, [7, -1, 7], 1.0)
    assert not r0["velocity_3d"].any() and np.all(r0["matched"] == -1)
    r1 = u(cam, p[::-1] + 1.0, [7, 9, -1], 1.5)  # 9: the caller numbered the -1 afterwards
    assert list(r1["matched"]) == [0, -1, -1] and r1["velocity_3d"][0].any() and not r1["velocity_3d"][1:].any()
    want = ((r1["un_pts_3d"][0] - r0["un_pts_3d"][0]).astype(np.float64) / 0.5).astype(np.float32)
    assert np.array_equal(r1["velocity_3d"][0], want)
    r2 = u(cam, p, [9, 7, 5], 1.5)  # dt = 0
    assert list(r2["matched"]) == [1, 0, -1] and not np.isfinite(r2["velocity_3d"][:2]).all() and not r2["velocity_3d"][2].any()
    u(cam, np.zeros((0, 2), np.float32), [], 2.0)
    r4 = u(cam, p, [9, 7, 5], 2.5)
    assert not r4["velocity_3d"].any() and np.all(r4["matched"] == -1)


# ---- track_plan.h behind a ctypes shim
SRC = r'''
#include "track_plan.h"
static LfvioCamera cam_of(const double *v) {
  LfvioCamera k;
  k.model = (int)v[0], k.cx = v[1], k.cy = v[2], k.c = v[3], k.d = v[4], k.e = v[5];
  for (int i = 0; i < 5; i++) k.poly[i] = v[6 + i];
  return k;
}
extern "C" const char *tp_reject(const double *cam, int N, const float *cur, const float *forw, int S, const int *samples) {
  LfvioCamera k = {};
  if (cam) k = cam_of(cam);
  LfvioTrackRejectIn in;
  in.camera = cam ? &k : nullptr, in.num_points = N, in.cur_pts = cur, in.forw_pts = forw, in.num_samples = S, in.samples = samples;
  return track_reject_check(&in);
}
extern "C" const char *tp_undistort(const double *cam, int N, const float *pts, const int *ids, double time) {
  LfvioCamera k = {};
  if (cam) k = cam_of(cam);
  LfvioTrackUndistortIn in;
  in.camera = cam ? &k : nullptr, in.num_points = N, in.pts = pts, in.ids = ids, in.time = time;
  return track_undistort_check(&in);
}
extern "C" void tp_cam(const double *cam, double *out) {
  const TrackCam t = track_cam(cam_of(cam));
  out[0] = t.cx, out[1] = t.cy, out[2] = t.c, out[3] = t.d, out[4] = t.e, out[5] = t.inv_scale;
  for (int i = 0; i < 5; i++) out[6 + i] = t.poly[i];
}
extern "C" int tp_consts(int *out) {
  const int v[] = {LFVIO_CAM_OCAM, LFVIO_TRACK_MAX_POINTS, TRACK_MAX_SAMPLES, TRACK_MIN_MATCHES, (int)sizeof(LfvioCamera),
                   (int)sizeof(LfvioTrackRejectIn), (int)sizeof(LfvioTrackRejectOut), (int)sizeof(LfvioTrackUndistortIn)};
  for (unsigned k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
  return (int)(sizeof v / sizeof v[0]);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="track_plan_")
    src, so = os.path.join(d, "tp.cpp"), os.path.join(d, "libtp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    so.tp_reject.restype = C.c_char_p
    so.tp_reject.argtypes = [dp, C.c_int, fp, fp, C.c_int, ip]
    so.tp_undistort.restype = C.c_char_p
    so.tp_undistort.argtypes = [dp, C.c_int, fp, ip, C.c_double]
    so.tp_cam.restype = None
    so.tp_cam.argtypes = [dp, dp]
    return so


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def test_plan_header_equals_the_restatements_checks(lib):
    pts = np.full((4096, 2), 100.0, np.float32)
    ids = np.arange(4096, dtype=np.int32)
    good = tr.make_samples(3, 40, 5)
    bad_hi, bad_lo, edge = good.copy(), good.copy(), good.copy()
    bad_hi[4, 7], bad_lo[0, 0], edge[2, 2] = 40, -1, 39
    other = dict(tr.PAL, model=1)
    cases = []  # (cam, N, cur, forw, S, samples)
    for cam in (tr.PAL, tr.SKEW, None, other):
        cases.append((cam, 40, pts, pts, 5, good))
    for N in (-1, 0, 1, 7, 8, 40, 4096, 4097):
        cases.append((tr.PAL, N, pts, pts, 5, good % max(min(N, 40), 1)))
        cases.append((tr.PAL, N, None, pts, 5, good % max(min(N, 40), 1)))
        cases.append((tr.PAL, N, pts, None, 5, good % max(min(N, 40), 1)))
        cases.append((tr.PAL, N, pts, pts, 5, None))
        cases.append((tr.PAL, N, pts, pts, 0, good % max(min(N, 40), 1)))
    for S in (-3, 0, 1, 5):
        cases.append((tr.PAL, 40, pts, pts, S, good))
    big = tr.make_samples(4, 40, 1025)
    cases += [(tr.PAL, 40, pts, pts, 1024, big), (tr.PAL, 40, pts, pts, 1025, big)]
    cases += [(tr.PAL, 40, pts, pts, 5, s) for s in (bad_hi, bad_lo, edge)]
    cases.append((tr.PAL, 39, pts, pts, 5, edge))  # the index 39 is outside [0, 39)
    refused = 0
    for cam, N, cur, forw, S, sm in cases:
        cv = None if cam is None else tr.cam_vector(cam)
        why = lib.tp_reject(_ptr(cv, C.c_double), N, _ptr(cur, C.c_float), _ptr(forw, C.c_float), S, _ptr(sm, C.c_int))
        want = tr.reject_check(cam, N, cur is not None, forw is not None, S, sm)
        assert (why is not None) == want, (cam is None, N, cur is None, forw is None, S, sm is None, why)
        assert why is None or why.startswith(b"lfvio_track"), why
        refused += want
    assert 10 < refused < len(cases)
    ucases = [(cam, 40, pts, ids, 1.0) for cam in (tr.PAL, tr.SKEW, None, other)]
    for N in (-1, 0, 1, 4096, 4097):
        ucases += [(tr.PAL, N, pts, ids, 1.0), (tr.PAL, N, None, ids, 1.0), (tr.PAL, N, pts, None, 1.0)]
    ucases += [(tr.PAL, 40, pts, ids, t) for t in (float("nan"), float("inf"), -float("inf"), 0.0, -5.0, 1e300)]
    refused = 0
    for cam, N, p, i, t in ucases:
        cv = None if cam is None else tr.cam_vector(cam)
        why = lib.tp_undistort(_ptr(cv, C.c_double), N, _ptr(p, C.c_float), _ptr(i, C.c_int), t)
        want = tr.undistort_check(cam, N, p is not None, i is not None, t)
        assert (why is not None) == want, (cam is None, N, p is None, i is None, t, why)
        refused += want
    assert 5 < refused < len(ucases)


def test_plan_header_camera_and_constants(lib):
    from lfvio import abi

    out = np.zeros(11)
    for cam in (tr.PAL, tr.SKEW, dict(tr.SKEW, c=0.3, d=7.0, e=-0.01)):
        cv = tr.cam_vector(cam)
        lib.tp_cam(_ptr(cv, C.c_double), _ptr(out, C.c_double))
        inv = np.float64(1.0) / (np.float64(cam["c"]) - np.float64(cam["d"]) * np.float64(cam["e"]))
        assert np.array_equal(out[:5], cv[1:6]) and np.array_equal(out[6:], cv[6:]) and out[5] == inv
    v = (C.c_int * 8)()
    assert lib.tp_consts(v) == 8
    assert list(v) == [abi.CAM_OCAM, abi.TRACK_MAX_POINTS, tr.MAX_SAMPLES, tr.MIN_MATCHES, C.sizeof(abi.CameraC), C.sizeof(abi.TrackRejectInC),
                       C.sizeof(abi.TrackRejectOutC), C.sizeof(abi.TrackUndistortInC)]
    assert (tr.CAM_OCAM, tr.MAX_POINTS) == (abi.CAM_OCAM, abi.TRACK_MAX_POINTS)


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi
    from lfvio.engine import Engine

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("lfvio_track_reject", "lfvio_track_undistort", "lfvio_track_reset"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+LFVIO_CAM_OCAM\s+0\b", src) and re.search(r"#define\s+LFVIO_TRACK_MAX_POINTS\s+4096\b", src)
    for name in ("track_reject", "track_undistort", "track_reset", "camera"):
        assert callable(getattr(Engine, name)), name
