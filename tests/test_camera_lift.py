"""Every camera model's lift on the CPU: lf-vio_amd/csrc/camera_models.h, compiled alone with g++ -ffp-contract=off behind a ctypes shim,
against its numpy texts bit for bit — tests/track_ref.py (OCam), tests/camera_ref.py (PINHOLE, MEI), tests/kb_ref.py (KANNALA_BRANDT),
chosen by the camera's model.  The cameras are all 13: PAL, SKEW, camera_ref.CAMERAS, kb_ref.CAMERAS; a camera travels as the 18 doubles
of test_kb_ref.vec18, every field its model does not read NaN.

  1  cam_lift and cam_bearing equal ref.lift / ref.bearings on every cur / forw array of track_cases.npz, camera_cases.npz and
     kb_cases.npz (and the bearings the fixtures record), on 4096 seeded float32 pixels per camera from 50 px outside the image on
     every side, and on the special pixels: the centre, +-0, +-3e38, +-inf, NaN and a denormal in either coordinate and in both.
     NaN positions are compared as a mask and every other value as bytes (IEEE 754 does not fix a NaN's payload); the special set is
     NaN in some rows and not in all, so the mask cannot hide a value
  2  cam_undistorted gives the un_pts and un_pts_3d that the three fixtures record for every call of every undistort sequence (all
     three gen_*.py record both, from ref.Undistort), as bytes
  3  every branch is reached: no_distortion on and off and xi == 1.0 / != 1.0 as track_cam forms them, the KANNALA_BRANDT fallback
     r > r_lim (RSFISH, on the wide pixels), r < 1e-10 there, and OCam's phi == 0: SKEW's centre is a float32 pixel and its bearing
     is exactly (0, 0, 1)
  4  (GPU) the device on the special pixels for the seven cameras that are not KANNALA_BRANDT (tests/test_kannala_brandt.py::test_lift
     does it for those): 32 + 32 pixels through lfvio_track_reject, the bearings against the numpy text, NaNs as a mask"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import camera_ref as cr
import kb_ref as kb
import track_ref as tr
from lfvio import synth
from test_kb_ref import bits, same_but_nan, vec18

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF, DENORMAL = float("nan"), float("inf"), 1e-40
REF = {0: tr, 2: cr, 3: cr, 5: kb}

# name -> (camera, (width, height))
CAMS = dict(PAL=(tr.PAL, (synth.OCAM_W, synth.OCAM_H)), SKEW=(tr.SKEW, (synth.OCAM_W, synth.OCAM_H)))
CAMS.update({n: (c, (cr.WIDTH, cr.HEIGHT)) for n, c in cr.CAMERAS.items()})
CAMS.update({n: (c, kb.SIZES[n]) for n, c in kb.CAMERAS.items()})
FIXTURES = (("track_cases.npz", tr), ("camera_cases.npz", cr), ("kb_cases.npz", kb))


def ref_of(cam):
    return REF[cam.get("model", 0)]


SRC = r'''
#include "camera_models.h"
static LfvioCamera cam_of(const double *v) {
  LfvioCamera k;
  k.model = (int)v[0], k.cx = v[1], k.cy = v[2], k.c = v[3], k.d = v[4], k.e = v[5];
  for (int i = 0; i < 5; i++) k.poly[i] = v[6 + i];
  k.fx = v[11], k.fy = v[12], k.k1 = v[13], k.k2 = v[14], k.p1 = v[15], k.p2 = v[16], k.xi = v[17];
  return k;
}
extern "C" int cl_branches(const double *cam) {
  const TrackCam t = track_cam(cam_of(cam));
  return t.no_distortion + 2 * (t.xi == 1.0);
}
extern "C" void cl_lift(const double *cam, int n, const float *px, double *P, double *b) {
  const TrackCam t = track_cam(cam_of(cam));
  for (int i = 0; i < n; i++) {
    const CamRay r = cam_lift(t, px[2 * i], px[2 * i + 1]);
    P[3 * i] = r.x, P[3 * i + 1] = r.y, P[3 * i + 2] = r.z;
    cam_bearing(t, px[2 * i], px[2 * i + 1], b + 3 * i);
  }
}
extern "C" void cl_undistorted(const double *cam, int n, const float *px, float *un, float *un3) {
  const TrackCam t = track_cam(cam_of(cam));
  for (int i = 0; i < n; i++) {
    const CamUndistorted u = cam_undistorted(t, px[2 * i], px[2 * i + 1]);
    un[2 * i] = u.ux, un[2 * i + 1] = u.uy, un3[3 * i] = u.bx, un3[3 * i + 1] = u.by, un3[3 * i + 2] = u.bz;
  }
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="camera_lift_")
    src, so = os.path.join(d, "cl.cpp"), os.path.join(d, "libcl.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    so.cl_branches.restype, so.cl_branches.argtypes = C.c_int, [dp]
    so.cl_lift.restype, so.cl_lift.argtypes = None, [dp, C.c_int, fp, dp, dp]
    so.cl_undistorted.restype, so.cl_undistorted.argtypes = None, [dp, C.c_int, fp, fp, fp]
    return so


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    """[(ref, arrays)] of the three .npz files: loaded once, shared, never changed."""
    out = []
    for name, ref in FIXTURES:
        z = np.load(os.path.join(golden_dir, name))
        out.append((ref, {k: z[k] for k in z.files}))
    return out


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def c_lift(lib, cam, px):
    """(P, bearing) of pixels px [N, 2] float32, from the header."""
    px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
    P, b = np.zeros((len(px), 3)), np.zeros((len(px), 3))
    lib.cl_lift(_p(vec18(cam)), len(px), _p(px, C.c_float), _p(P), _p(b))
    return P, b


def wide_pixels(name):
    W, H = CAMS[name][1]
    rng = np.random.default_rng([8, list(CAMS).index(name)])
    return rng.uniform([-50.0, -50.0], [W + 50.0, H + 50.0], (4096, 2)).astype(np.float32)


def special_pixels(cam):
    """48 pixels: the centre; +-0, +-3e38, +-inf, NaN and a denormal in either coordinate beside the centre's other one; NaN, +-inf and
    +-3e38 in both, every pair; zeros and denormals in both."""
    c = [cam["cx"], cam["cy"]]
    odd = [NAN, INF, -INF, 3e38, -3e38]
    one = odd + [0.0, -0.0, DENORMAL]
    px = [c] + [[v, c[1]] for v in one] + [[c[0], v] for v in one] + [[v, w] for v in odd for w in odd]
    px += [[0.0, 0.0], [-0.0, -0.0], [DENORMAL, DENORMAL], [-0.0, 0.0], [DENORMAL, -0.0], [0.0, -DENORMAL]]
    return np.array(px, np.float32)


def holds(lib, cam, px, tag):
    """The header's lift and bearing of px against the camera's numpy text; returns the text's bearings."""
    ref = ref_of(cam)
    P, b = c_lift(lib, cam, px)
    want = ref.bearings(cam, px)
    assert same_but_nan(P, ref.lift(cam, px)), tag
    assert same_but_nan(b, want), tag
    return want


# ---- 1
def test_lift_on_the_fixtures(lib, fixtures):
    n, recorded = 0, 0
    for ref, fx in fixtures:
        for name in fx["names"]:
            cam = ref.cam_from_vector(fx[f"{name}/cam"])
            assert ref_of(cam) is ref, name
            for key in ("cur", "forw"):
                b = holds(lib, cam, fx[f"{name}/{key}"], (name, key))
                assert np.isfinite(b).all(), name
                if f"{name}/bearing_{key}" in fx:
                    assert np.array_equal(bits(c_lift(lib, cam, fx[f"{name}/{key}"])[1]), bits(fx[f"{name}/bearing_{key}"])), (name, key)
                    recorded += 1
                n += 1
    assert n == 2 * (len(tr.CASES) + len(cr.CASES) + len(kb.CASES)) and recorded == n - 2 * 3  # (one case of fewer than 8 matches each)


def test_lift_on_wide_and_special_pixels(lib):
    assert len(CAMS) == 13
    for name, (cam, _) in CAMS.items():
        px = wide_pixels(name)
        assert px[:, 0].min() < -40 and px[:, 1].min() < -40
        holds(lib, cam, px, name)
        sp = special_pixels(cam)
        want = holds(lib, cam, sp, name)
        rows = np.isnan(want).any(axis=1)
        assert len(sp) == 48 and rows.any() and not rows.all() and np.isfinite(want[0]).all(), name


# ---- 2
def test_undistorted_equals_the_fixtures(lib, fixtures):
    calls = 0
    for ref, fx in fixtures:
        for s in fx["sequences"]:
            cam = ref.cam_from_vector(fx[f"{s}/cam"])
            for j in range(int(fx[f"{s}/calls"])):
                pts = np.ascontiguousarray(fx[f"{s}/{j}/pts"], np.float32)
                un, un3 = np.zeros((len(pts), 2), np.float32), np.zeros((len(pts), 3), np.float32)
                lib.cl_undistorted(_p(vec18(cam)), len(pts), _p(pts, C.c_float), _p(un, C.c_float), _p(un3, C.c_float))
                assert np.array_equal(bits(un), bits(fx[f"{s}/{j}/un_pts"])), (s, j)
                assert np.array_equal(bits(un3), bits(fx[f"{s}/{j}/un_pts_3d"])), (s, j)
                calls += 1
    assert calls == 4 * 13


# ---- 3
def test_every_branch_is_reached(lib):
    flags = {name: lib.cl_branches(_p(vec18(cam))) for name, (cam, _) in CAMS.items()}
    assert [flags[n] for n in ("EUROC", "MV3DM", "EUROC_ND", "MV3DM_ND", "MEI_XI1")] == [0, 0, 1, 1, 2], flags  # no_distortion + 2 (xi == 1.0)
    assert cr.MEI_XI1["xi"] == 1.0 and cr.MV3DM["xi"] != 1.0 and cr.host_constants(cr.EUROC_ND)["no_distortion"]
    # KANNALA_BRANDT: the fallback on RSFISH's wide pixels and nowhere on TUM's; r < 1e-10 on a camera whose centre is a float32 pixel
    hit = {n: int(kb.fell_back(kb.CAMERAS[n], kb.plane(kb.CAMERAS[n], wide_pixels(n))[2]).sum()) for n in ("RSFISH", "TUM")}
    assert hit["RSFISH"] > 0 and hit["TUM"] == 0, hit
    centred, px = dict(kb.TUM, cx=255.5, cy=256.25), np.array([[255.5, 256.25]], np.float32)
    assert 0.0 < kb.plane(centred, px)[2][0] < 1e-10
    holds(lib, centred, px, "centred")
    # OCam, phi == 0: the polynomial's constant term alone, and the bearing is the axis
    px = np.array([[tr.SKEW["cx"], tr.SKEW["cy"]]], np.float32)
    assert px[0, 0] == tr.SKEW["cx"] and px[0, 1] == tr.SKEW["cy"]
    P, b = c_lift(lib, tr.SKEW, px)
    assert P[0].tolist() == [0.0, 0.0, -tr.SKEW["poly"][0]] and b[0].tolist() == [0.0, 0.0, 1.0]
    assert same_but_nan(b, tr.bearings(tr.SKEW, px))


# ---- 4
@pytest.mark.gpu
def test_special_pixels_on_the_device(eng):
    n = 0
    for name, (cam, _) in CAMS.items():
        if ref_of(cam) is kb:
            continue
        sp = special_pixels(cam)
        px = np.concatenate([sp, sp[::-1]])[:64]
        d = eng.track_reject(cam, px[:32], px[32:], tr.make_samples(1, 32, 1), want_bearings=True)
        for got, want in ((d["bearing_cur"], ref_of(cam).bearings(cam, px[:32])), (d["bearing_forw"], ref_of(cam).bearings(cam, px[32:]))):
            assert np.isnan(want).any() and not np.isnan(want).all() and same_but_nan(got, want), name
        n += 1
    assert n == 7
