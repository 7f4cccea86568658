"""Every camera model's projection on the CPU: lf-vio_amd/csrc/camera_models.h + camera_atan.h, compiled alone with g++ -ffp-contract=off
-Wall -Werror behind a ctypes shim, against the numpy text tests/project_ref.py bit for bit.  The cameras are the 13 of
tests/test_camera_lift.py (the OCam pair with its inverse polynomial); a camera travels as the 18 doubles of test_kb_ref.vec18, every
field its model does not read NaN, and the 20 of inv_poly.

  1  cam_atan equals project_ref.atan as bytes on the points of test_project_ref.atan_points and on +-0, +-inf, NaN
  2  cam_project equals project_ref.project — NaN positions as a mask, every other value as bytes — on the fixture's rays (and gives
     the pixels tests/golden/remap_cases.npz records), on 4096 seeded rays per camera over the whole sphere (z < 0 included) and on
     the special rays: the zero vector, the optical axis and its negative, X = Y = 0, Z = 0, +-inf, NaN and a denormal in each
     component.  The special set is NaN in some rows and not in all, so the mask cannot hide a value
  3  every branch is reached: no_distortion on and off, xi == 1.0 and != 1.0 as proj_cam forms them, KANNALA_BRANDT's Z > 0, Z < 0,
     Z == 0 and rxy < 1e-10, OCam's n == 0 (NaN, as the reference's 0 * inf)
  4  proj_cam and proj_check: fx, fy as given, the inverse polynomial for OCam alone, TrackCam's members what track_cam gives; a
     non-finite inv_poly entry is refused for OCam and not looked at for the other models"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import camera_ref as cr
import project_ref as pr
import test_project_ref as tpr
from test_kb_ref import bits, same_but_nan, vec18

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

SRC = r'''
#include "camera_models.h"
static LfvioCamera cam_of(const double *v) {
  LfvioCamera k;
  k.model = (int)v[0], k.cx = v[1], k.cy = v[2], k.c = v[3], k.d = v[4], k.e = v[5];
  for (int i = 0; i < 5; i++) k.poly[i] = v[6 + i];
  k.fx = v[11], k.fy = v[12], k.k1 = v[13], k.k2 = v[14], k.p1 = v[15], k.p2 = v[16], k.xi = v[17];
  return k;
}
static LfvioProjector proj_of(const LfvioCamera *k, const double *inv) {
  LfvioProjector p;
  p.camera = k;
  for (int i = 0; i < LFVIO_OCAM_INV_POLY_SIZE; i++) p.inv_poly[i] = inv[i];
  return p;
}
extern "C" void cp_atan(int n, const double *x, double *y) {
  for (int i = 0; i < n; i++) y[i] = cam_atan(x[i]);
}
extern "C" void cp_project(const double *cam, const double *inv, int n, const double *P, double *px) {
  const LfvioCamera k = cam_of(cam);
  const ProjCam q = proj_cam(proj_of(&k, inv));
  for (int i = 0; i < n; i++) {
    const CamPixel p = cam_project(q, P[3 * i], P[3 * i + 1], P[3 * i + 2]);
    px[2 * i] = p.u, px[2 * i + 1] = p.v;
  }
}
// fx, fy, inv_poly[20], then no_distortion, xi == 1.0, and whether the TrackCam inside equals track_cam's, byte for byte of its members
extern "C" void cp_cam(const double *cam, const double *inv, double *out) {
  const LfvioCamera k = cam_of(cam);
  const ProjCam q = proj_cam(proj_of(&k, inv));
  const TrackCam t = track_cam(k);
  out[0] = q.fx, out[1] = q.fy;
  for (int i = 0; i < CAM_INV_POLY; i++) out[2 + i] = q.inv_poly[i];
  out[22] = q.t.no_distortion, out[23] = q.t.xi == 1.0;
  const double a[] = {q.t.cx, q.t.cy, q.t.c, q.t.d, q.t.e, q.t.inv_scale, q.t.inv11, q.t.inv13, q.t.inv22, q.t.inv23, q.t.k1, q.t.k2, q.t.p1, q.t.p2, q.t.xi, q.t.theta_lim, q.t.r_lim};
  const double b[] = {t.cx, t.cy, t.c, t.d, t.e, t.inv_scale, t.inv11, t.inv13, t.inv22, t.inv23, t.k1, t.k2, t.p1, t.p2, t.xi, t.theta_lim, t.r_lim};
  out[24] = std::memcmp(a, b, sizeof a) == 0 && std::memcmp(q.t.poly, t.poly, sizeof t.poly) == 0 && q.t.model == t.model && q.t.no_distortion == t.no_distortion;
}
extern "C" const char *cp_check(const double *cam, const double *inv, int null_camera) {
  const LfvioCamera k = cam_of(cam);
  const LfvioProjector p = proj_of(null_camera ? nullptr : &k, inv);
  return proj_check(&p);
}
extern "C" const char *cp_check_null() { return proj_check(nullptr); }
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="camera_project_")
    src, so = os.path.join(d, "cp.cpp"), os.path.join(d, "libcp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    so.cp_atan.restype, so.cp_atan.argtypes = None, [C.c_int, dp, dp]
    so.cp_project.restype, so.cp_project.argtypes = None, [dp, dp, C.c_int, dp, dp]
    so.cp_cam.restype, so.cp_cam.argtypes = None, [dp, dp, dp]
    so.cp_check.restype, so.cp_check.argtypes = C.c_char_p, [dp, dp, C.c_int]
    so.cp_check_null.restype, so.cp_check_null.argtypes = C.c_char_p, []
    return so


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "remap_cases.npz"))
    return {k: z[k] for k in z.files}


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def inv20(cam):
    """The 20 of inv_poly; NaN for a model that must not read them."""
    return pr.inv_poly_of(cam) if pr.model_of(cam) == 0 else np.full(20, NAN)


def c_project(lib, cam, P):
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    px = np.zeros((len(P), 2))
    lib.cp_project(_p(vec18(cam)), _p(inv20(cam)), len(P), _p(P), _p(px))
    return px


def holds(lib, cam, P, tag):
    want = pr.project(cam, P)
    assert same_but_nan(c_project(lib, cam, P), want), tag
    return want


# ---- 1
def test_atan_equals_the_text(lib):
    x = np.concatenate([tpr.atan_points(), [0.0, -0.0, np.inf, -np.inf, NAN]])
    y = np.zeros_like(x)
    lib.cp_atan(len(x), _p(x), _p(y))
    assert same_but_nan(y, pr.atan(x))
    assert np.signbit(y[-4]) and y[-4] == 0.0 and y[-3] == np.pi / 2 and y[-2] == -np.pi / 2 and np.isnan(y[-1])


# ---- 2
def test_project_on_the_fixture(lib, fx):
    assert list(fx["names"]) == list(pr.CAMS) and len(pr.CAMS) == 13
    for name in fx["names"]:
        cam = pr.cam_from_vector(fx[f"{name}/cam"])
        assert np.array_equal(bits(pr.cam_vector(cam)), bits(pr.cam_vector(pr.CAMS[name][0]))), name
        want = holds(lib, cam, fx[f"{name}/P"], name)
        assert same_but_nan(want, fx[f"{name}/px"]) and np.isfinite(want[:24]).all(), name


def test_project_over_the_sphere_and_on_special_rays(lib):
    sp = pr.special_rays()
    for name, (cam, _) in pr.CAMS.items():
        P = pr.sphere_rays(name)
        assert len(P) == 4096 and (P[:, 2] < 0).sum() > 1500
        holds(lib, cam, P, name)
        want = holds(lib, cam, sp, name)
        rows = np.isnan(want).any(axis=1)
        assert rows.any() and not rows.all() and np.isnan(want[0]).all(), name  # (the zero vector is NaN for every model)


# ---- 3
def test_every_branch_is_reached(lib):
    out = {}
    for name, (cam, _) in pr.CAMS.items():
        o = np.zeros(25)
        lib.cp_cam(_p(vec18(cam)), _p(inv20(cam)), _p(o))
        out[name] = o
    assert [(int(out[n][22]), int(out[n][23])) for n in ("EUROC", "MV3DM", "EUROC_ND", "MV3DM_ND", "MEI_XI1")] == [(0, 0), (0, 0), (1, 0), (1, 0), (0, 1)]
    assert cr.MEI_XI1["xi"] == 1.0 and pr.no_distortion(cr.EUROC_ND) and not pr.no_distortion(cr.EUROC)
    # KANNALA_BRANDT: the three cases of Z and rxy < 1e-10, each among the special rays and each finite
    sp = pr.special_rays()
    fin = np.isfinite(sp).all(axis=1)
    rxy = np.hypot(sp[:, 0], sp[:, 1])
    cases = dict(front=fin & (sp[:, 2] > 0) & (rxy >= 1e-10), back=fin & (sp[:, 2] < 0) & (rxy >= 1e-10), side=fin & (sp[:, 2] == 0) & (rxy >= 1e-10),
                 axis=fin & (rxy < 1e-10) & (sp[:, 2] != 0), tiny_side=fin & (rxy < 1e-10) & (rxy > 0) & (sp[:, 2] == 0))
    tum = pr.CAMS["TUM"][0]
    px = c_project(lib, tum, sp)
    for k, m in cases.items():
        assert m.any() and np.isfinite(px[m]).all(), k
    on_axis = cases["axis"] & (sp[:, 2] > 0) & (rxy == 0)
    assert on_axis.any() and (px[on_axis] == [tum["cx"], tum["cy"]]).all()  # theta = 0, r = 0
    back = np.array([[0.0, 0.0, -1.0]])
    assert c_project(lib, tum, back)[0, 1] == tum["cy"] and c_project(lib, tum, back)[0, 0] > tum["cx"]  # theta = pi, phi = 0
    # OCam: n == 0 is NaN (0 * inf), as in the reference; just off the axis it is finite
    pal = pr.CAMS["PAL"][0]
    assert np.isnan(c_project(lib, pal, [[0.0, 0.0, 1.0], [0.0, 0.0, -2.0]])).all()
    assert np.isfinite(c_project(lib, pal, [[1e-11, 0.0, -1.0]])).all()


# ---- 4
def test_proj_cam_and_proj_check(lib):
    for name, (cam, _) in pr.CAMS.items():
        o = np.zeros(25)
        lib.cp_cam(_p(vec18(cam)), _p(inv20(cam)), _p(o))
        assert o[24] == 1.0, name
        if pr.model_of(cam) == 0:
            assert o[0] == 0.0 and o[1] == 0.0 and np.array_equal(bits(o[2:22]), bits(pr.inv_poly_of(cam))), name
        else:
            assert o[0] == cam["fx"] and o[1] == cam["fy"] and (o[2:22] == 0.0).all(), name
        assert lib.cp_check(_p(vec18(cam)), _p(inv20(cam)), 0) is None, name
        assert not pr.projector_check(cam), name
    pal = pr.CAMS["PAL"][0]
    for k in (0, 13, 19):
        for bad in (NAN, np.inf, -np.inf):
            inv = pr.inv_poly_of(pal)
            inv[k] = bad
            assert lib.cp_check(_p(vec18(pal)), _p(inv), 0) is not None and pr.projector_check(dict(pal, inv_poly=tuple(inv)))
    assert lib.cp_check(_p(vec18(pal)), _p(pr.inv_poly_of(pal)), 1) is not None and lib.cp_check_null() is not None
    euroc = pr.CAMS["EUROC"][0]
    assert lib.cp_check(_p(vec18(dict(euroc, fx=0.0))), _p(inv20(euroc)), 0) is not None and pr.projector_check(dict(euroc, fx=0.0))
    assert lib.cp_check(_p(vec18(dict(euroc, model=4))), _p(inv20(euroc)), 0) is not None and pr.projector_check(dict(euroc, model=4))
