"""CPU tests of the KANNALA_BRANDT camera model's specification (tests/kb_ref.py), its fixture (tests/golden/kb_cases.npz) and the plain
C++ of lf-vio_amd/csrc/camera_kb.h + track_plan.h, compiled alone with g++ -ffp-contract=off.

  1  C++ equals numpy, bit for bit: theta_lim, r_lim, the inv values and the whole TrackCam of every camera (with and without the
     constants' cache, and across a change of camera); the lift on every fixture case, on 2 x 1031 pixels over and 50 px beyond the
     image (RSFISH reaches r > r_lim there: the fallback is hit, asserted) and on the special pixels: the principal point, r < 1e-10,
     NaN, +-inf, +-3e38 — NaN positions as a mask, everything else as bytes
  2  the specification against 50 digits (mpmath): per camera r swept over [0, min(r at the corner + 50 px, r_lim)] (129 points, as
     points (r cos phi, r sin phi) of the plane) plus, where r_lim is within reach, the 200 points r_lim (1 - 10^-16 .. 10^-2).  The
     reference root is mpmath.polyroots with the reference's own filter (|imag| <= 1e-10, real >= -1e-10, negative clamped to 0,
     the minimum).  The bars are four times the worst value the restatement reaches on this sweep (measured):
       (a) residual |f(theta) - r| / (eps r)                                         measured 0.89   bar 3.6
       (b) root     |theta - theta*| f'(theta*) / (eps max(theta*, r)), f' >= 0.1    measured 0.89   bar 3.6
       (c) sin, cos on 10^4 points of [0, pi], the quadrant boundaries among them    measured 1.37   bar 5.4 ulp
       (d) the angle between the unit bearing and the 50-digit one, f' >= 0.1        measured 6.4    bar 25.6 eps
     (d) is (b) seen from the ray: an error of 0.9 eps max(theta, r) / f' in theta is up to 14 eps of angle where f' = 0.1 and
     theta = 1.6 (RSFISH, the worst), and 5.4 eps at TUM's theta = 2.7; where f' is 1 it is 1.2 eps.
     and NEWTON_STEPS is the largest step count the sweep needs to get under bar (a), 11, plus two.  Where the reference's filter
     finds no root the specification took the fallback.
  3  lift(project(ray)) gives the ray's direction back to 1e-9 inside each camera's field of view
  4  branches: KB_IDEAL gives theta == r exactly; KB_K5_0 and KB_K45_0 are held to bars (a) and (c)/(d) in the sweep of test 2
  5  the checks: every refused field alone, every accepted camera, models 1, 4, 7, -1 still refused, an OCam / PINHOLE / MEI camera
     with NaN in the fields it does not read accepted with the TrackCam members it had
  6  the fixture regenerates from its seeds; no RANSAC case breaks C1 / C2, so none would drop out of the GPU test's comparison"""
import ctypes as C
import os
import subprocess
import tempfile

import mpmath as mp
import numpy as np
import pytest

import camera_ref as cr
import kb_ref as kb
import track_ref as tr
from golden import gen_kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
BAR_RESIDUAL, BAR_ROOT, BAR_SINCOS, BAR_ANGLE = 3.6, 3.6, 5.4, 25.6
NAN, INF = float("nan"), float("inf")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiub" else a


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "kb_cases.npz"))
    return {k: z[k] for k in z.files}


# ---- the C++ behind a ctypes shim.  A camera travels as 18 doubles: model, cx, cy, c, d, e, poly[5], fx, fy, k1, k2, p1, p2, xi
SRC = r'''
#include "track_plan.h"
static LfvioCamera cam_of(const double *v) {
  LfvioCamera k;
  k.model = (int)v[0], k.cx = v[1], k.cy = v[2], k.c = v[3], k.d = v[4], k.e = v[5];
  for (int i = 0; i < 5; i++) k.poly[i] = v[6 + i];
  k.fx = v[11], k.fy = v[12], k.k1 = v[13], k.k2 = v[14], k.p1 = v[15], k.p2 = v[16], k.xi = v[17];
  return k;
}
static void put(const TrackCam &t, double *out) {
  out[0] = t.cx, out[1] = t.cy, out[2] = t.c, out[3] = t.d, out[4] = t.e, out[5] = t.inv_scale;
  for (int i = 0; i < 5; i++) out[6 + i] = t.poly[i];
  out[11] = t.inv11, out[12] = t.inv13, out[13] = t.inv22, out[14] = t.inv23;
  out[15] = t.k1, out[16] = t.k2, out[17] = t.p1, out[18] = t.p2, out[19] = t.xi, out[20] = t.model, out[21] = t.no_distortion;
  out[22] = t.theta_lim, out[23] = t.r_lim;
}
static KbCache cache;
extern "C" const char *kt_check(const double *cam, int N) {
  const LfvioCamera k = cam_of(cam);
  return track_common_check(&k, N);
}
extern "C" void kt_cam(const double *cam, int cached, double *out) { put(track_cam(cam_of(cam), cached ? &cache : nullptr), out); }
extern "C" int kt_cache_valid() { return cache.valid; }
extern "C" void kt_cache_poison() { cache.c.theta_lim = -1.0, cache.c.r_lim = -2.0; }  // a hit returns these, a miss overwrites them
extern "C" void kt_lift(const double *cam, int n, const float *px, double *P) {
  const TrackCam t = track_cam(cam_of(cam));
  for (int i = 0; i < n; i++)
    kb_lift_pixel(t.inv11, t.inv13, t.inv22, t.inv23, t.poly, t.theta_lim, t.r_lim, px[2 * i], px[2 * i + 1], P[3 * i], P[3 * i + 1], P[3 * i + 2]);
}
extern "C" void kt_root(const double *cam, int n, const double *r, double *th) {
  const TrackCam t = track_cam(cam_of(cam));
  for (int i = 0; i < n; i++) th[i] = kb_root(t.poly, t.theta_lim, t.r_lim, r[i]);
}
extern "C" void kt_sincos(int n, const double *th, double *s, double *c) {
  for (int i = 0; i < n; i++) kb_sincos(th[i], s[i], c[i]);
}
extern "C" void kt_consts(int *out) {
  out[0] = LFVIO_CAM_KANNALA_BRANDT, out[1] = (int)sizeof(LfvioCamera), out[2] = (int)sizeof(TrackCam), out[3] = KB_NEWTON_STEPS, out[4] = KB_GRID;
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="kb_plan_")
    src, so = os.path.join(d, "kt.cpp"), os.path.join(d, "libkt.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    so.kt_check.restype = C.c_char_p
    so.kt_check.argtypes = [dp, C.c_int]
    so.kt_cam.restype = so.kt_lift.restype = so.kt_root.restype = so.kt_sincos.restype = so.kt_consts.restype = so.kt_cache_poison.restype = None
    so.kt_cam.argtypes = [dp, C.c_int, dp]
    so.kt_lift.argtypes = [dp, C.c_int, fp, dp]
    so.kt_root.argtypes = [dp, C.c_int, dp, dp]
    so.kt_sincos.argtypes = [C.c_int, dp, dp, dp]
    so.kt_consts.argtypes = [ip]
    return so


def vec18(cam):
    """The 18 doubles of the shim; what the model does not read is NaN: a field the header must not look at."""
    if cam.get("model", 0) != kb.CAM_KANNALA_BRANDT:
        poly = cam.get("poly", (NAN,) * 5)
        return np.array([cam.get("model", 0), cam["cx"], cam["cy"], cam.get("c", NAN), cam.get("d", NAN), cam.get("e", NAN), *poly,
                         *[cam.get(k, NAN) for k in ("fx", "fy", "k1", "k2", "p1", "p2", "xi")]], np.float64)
    return np.array([cam["model"], cam["cx"], cam["cy"], NAN, NAN, NAN, cam["k2"], cam["k3"], cam["k4"], cam["k5"], NAN, cam["fx"], cam["fy"],
                     NAN, NAN, NAN, NAN, NAN], np.float64)


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def track_cam(lib, cam, cached=0):
    out = np.full(24, -7.0)
    lib.kt_cam(_p(vec18(cam)), cached, _p(out))
    return out


def want_cam(cam):
    h = kb.host_constants(cam)
    return np.array([cam["cx"], cam["cy"], 0, 0, 0, 0, cam["k2"], cam["k3"], cam["k4"], cam["k5"], 0, h["inv11"], h["inv13"], h["inv22"], h["inv23"],
                     0, 0, 0, 0, 0, 5, 0, h["theta_lim"], h["r_lim"]], np.float64)


def c_lift(lib, cam, px):
    px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
    P = np.zeros((len(px), 3))
    lib.kt_lift(_p(vec18(cam)), len(px), _p(px, C.c_float), _p(P))
    return P


def same_but_nan(got, want):
    """NaN positions as a mask (x86 and gfx950 make NaNs of opposite sign), every other value as bytes."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def wide_pixels(name):
    W, H = kb.SIZES[name]
    return np.random.default_rng(8).uniform([-50.0, -50.0], [W + 50.0, H + 50.0], (2 * 1031, 2)).astype(np.float32)


def special_pixels(cam):
    """The principal point (as the nearest float32 pixel and, for r < 1e-10, a camera is made whose centre IS one: see the test),
    NaN, +-inf and +-3e38 in either coordinate and both."""
    c = [cam["cx"], cam["cy"]]
    odd = [NAN, INF, -INF, 3e38, -3e38]
    px = [c] + [[v, c[1]] for v in odd] + [[c[0], v] for v in odd] + [[v, w] for v in odd for w in odd]
    return np.array(px, np.float32)


# ---- 1
def test_constants_and_track_cam(lib):
    v = (C.c_int * 5)()
    lib.kt_consts(v)
    from lfvio import abi, synth

    assert list(v)[:2] == [abi.CAM_KANNALA_BRANDT, C.sizeof(abi.CameraC)] and v[2] % 8 == 0
    assert v[3] == kb.NEWTON_STEPS and v[4] == kb.GRID and kb.CAM_KANNALA_BRANDT == abi.CAM_KANNALA_BRANDT == synth.CAM_KANNALA_BRANDT == 5
    for name, cam in kb.CAMERAS.items():
        t, want = track_cam(lib, cam), want_cam(cam)
        assert np.array_equal(bits(t), bits(want)), (name, t, want)
        c = abi.camera_c(cam)
        assert (c.model, c.cx, c.cy, c.fx, c.fy, list(c.poly), c.k1, c.k2, c.xi) == (
            5, cam["cx"], cam["cy"], cam["fx"], cam["fy"], [cam["k2"], cam["k3"], cam["k4"], cam["k5"], 0.0], 0.0, 0.0, 0.0), name
    h = {n: kb.host_constants(c) for n, c in kb.CAMERAS.items()}
    assert h["TUM"]["theta_lim"] == h["CLA"]["theta_lim"] == h["KB_IDEAL"]["theta_lim"] == np.pi and h["KB_IDEAL"]["r_lim"] == np.pi
    assert abs(h["RSFISH"]["theta_lim"] - 1.6176) < 1e-4 and abs(h["RSFISH"]["r_lim"] - 1.50758) < 1e-5
    # the cache: the first call fills it, a second call with the same camera is a hit (the poisoned constants come back), another
    # camera is a miss, and the constants follow it
    assert not lib.kt_cache_valid()
    assert np.array_equal(bits(track_cam(lib, kb.TUM, 1)), bits(want_cam(kb.TUM))) and lib.kt_cache_valid()
    lib.kt_cache_poison()
    assert list(track_cam(lib, kb.TUM, 1)[22:]) == [-1.0, -2.0]
    assert np.array_equal(bits(track_cam(lib, kb.RSFISH, 1)), bits(want_cam(kb.RSFISH)))
    assert np.array_equal(bits(track_cam(lib, kb.TUM, 1)), bits(want_cam(kb.TUM)))
    lib.kt_cache_poison()
    assert np.array_equal(bits(track_cam(lib, dict(kb.TUM, k5=-kb.TUM["k5"]), 1)), bits(want_cam(dict(kb.TUM, k5=-kb.TUM["k5"]))))
    lib.kt_cache_poison()  # another model neither reads nor fills it
    assert np.array_equal(track_cam(lib, cr.EUROC, 1)[22:], [0.0, 0.0]) and list(track_cam(lib, dict(kb.TUM, k5=-kb.TUM["k5"]), 1)[22:]) == [-1.0, -2.0]


def test_lift_equals_numpy(lib, fx):
    n = 0
    for name in kb.CASES:
        cam = kb.cam_from_vector(fx[f"{name}/cam"])
        for key in ("cur", "forw"):
            px = fx[f"{name}/{key}"]
            assert np.array_equal(bits(c_lift(lib, cam, px)), bits(kb.lift(cam, px))), (name, key)
            n += len(px)
    assert n >= 500
    hit = {}
    for name, cam in kb.CAMERAS.items():
        px = wide_pixels(name)
        got, want = c_lift(lib, cam, px), kb.lift(cam, px)
        assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want)), name
        hit[name] = int(kb.fell_back(cam, kb.plane(cam, px)[2]).sum())
        sp = special_pixels(cam)
        got, want = c_lift(lib, cam, sp), kb.lift(cam, sp)
        assert np.isnan(want).any() and np.isfinite(want[0]).all() and same_but_nan(got, want), name
    assert hit["RSFISH"] > 0 and hit["TUM"] == 0 and hit["CLA"] == 0, hit  # the fallback branch is reached, and only where expected
    # r < 1e-10: a camera whose centre is a float32 pixel.  inv11 px + inv13 leaves a rounding residue (r is 2e-16 here, not 0), and
    # the branch of :722-725 takes phi = 0 whatever y is: P = (sin theta, 0, cos theta) with theta = r
    centred = dict(kb.TUM, cx=255.5, cy=256.25)
    px = np.array([[255.5, 256.25]], np.float32)
    want, (x, y, r) = kb.lift(centred, px), kb.plane(centred, px)
    assert 0.0 < r[0] < 1e-10 and want[0, 1] == 0.0 and want[0, 2] == 1.0
    assert want[0, 0] == kb.sincos(r)[0][0] and abs(want[0, 0]) < 1e-10
    assert np.array_equal(bits(c_lift(lib, centred, px)), bits(want))
    # the root and the sin / cos alone, far outside what a pixel gives
    th = np.concatenate([np.linspace(0.0, 40.0, 4001), [1e6, 1e15, 1e22, 3e38, 1e300, INF, NAN]])
    s, c = np.zeros_like(th), np.zeros_like(th)
    lib.kt_sincos(len(th), _p(th), _p(s), _p(c))
    ws, wc = kb.sincos(th)
    assert same_but_nan(s, ws) and same_but_nan(c, wc) and np.isfinite(ws[:4003]).all()
    for name, cam in kb.CAMERAS.items():
        r = np.concatenate([np.linspace(0.0, 4.0, 2001), [1e-300, 1e-12, 1e6, 3e38, INF, NAN]])
        got = np.zeros_like(r)
        lib.kt_root(_p(vec18(cam)), len(r), _p(r), _p(got))
        assert same_but_nan(got, kb.root(cam, r)), name


# ---- 2: 50 digits
mp.mp.dps = 50


def mk(cam):
    return [mp.mpf(float(cam[x])) for x in ("k2", "k3", "k4", "k5")]


def f_mp(k, th):
    t = th * th
    return th * (1 + t * (k[0] + t * (k[1] + t * (k[2] + t * k[3]))))


def fp_mp(k, th):
    t = th * th
    return 1 + t * (3 * k[0] + t * (5 * k[1] + t * (7 * k[2] + t * 9 * k[3])))


def reference_root(cam, r):
    """backprojectSymmetric's theta in 50 digits: the roots of the polynomial of the degree the reference forms (:730-768), its
    filter (:786-806), the minimum; None where the filter leaves nothing (the reference then takes theta = r, :809-812)."""
    k = mk(cam)
    co = [k[3], 0, k[2], 0, k[1], 0, k[0], 0, mp.mpf(1), -mp.mpf(float(r))]
    while co[0] == 0 and len(co) > 2:
        co = co[2:]
    if len(co) == 2:
        return mp.mpf(float(r))  # npow == 1 (:771-774)
    ok = []
    for z in mp.polyroots(co, maxsteps=200, extraprec=200):
        if abs(mp.im(z)) > 1e-10 or mp.re(z) < -1e-10:
            continue
        ok.append(max(mp.re(z), mp.mpf(0)))
    return min(ok) if ok else None


def ulps(exact, got):
    return float(abs(exact - mp.mpf(float(got))) / mp.mpf(float(np.spacing(abs(got)))))


@pytest.fixture(scope="module")
def sweep():
    """Per camera: the swept points of the plane, the specification's r, theta and bearing there, and the 50-digit roots.  Computed
    once, shared by tests 2 and 4, never changed."""
    out = {}
    for name, cam in kb.CAMERAS.items():
        h = kb.host_constants(cam)
        W, H = kb.SIZES[name]
        corners = np.array([[-50, -50], [W + 50, -50], [-50, H + 50], [W + 50, H + 50]], np.float32)
        rc, rl = float(kb.plane(cam, corners, h)[2].max()), float(h["r_lim"])
        r0 = np.linspace(0.0, min(rc, rl), 129)
        phi = np.random.default_rng(3).uniform(0.0, 2 * np.pi, len(r0))
        x, y = r0 * np.cos(phi), r0 * np.sin(phi)
        if rl <= rc:  # r_lim is within reach: on the x axis, where sqrt(r r) == r
            near = rl * (1.0 - np.logspace(-16, -2, 200))
            x, y = np.concatenate([x, near]), np.concatenate([y, np.zeros(200)])
        r = np.sqrt(x * x + y * y)
        r = np.where(r <= rl, r, rl)
        x = np.where(y == 0.0, r, x)
        out[name] = dict(cam=cam, h=h, x=x, y=y, r=np.sqrt(x * x + y * y), within=rl <= rc, ref=None)
        s = out[name]
        assert (s["r"] <= rl).all()
        s["theta"] = kb.root(cam, s["r"], h=h)
        s["ref"] = [reference_root(cam, v) for v in s["r"]]
    return out


def measure(s, steps=kb.NEWTON_STEPS):
    """(a), (b), (d) over a camera's sweep: the worst values."""
    cam, k = s["cam"], mk(s["cam"])
    th = kb.root(cam, s["r"], steps=steps, h=s["h"])
    res = max((float(abs(f_mp(k, mp.mpf(float(t))) - mp.mpf(float(r))) / (EPS * r)) if r > 0 else float(t != 0)) for t, r in zip(th, s["r"]))
    if steps != kb.NEWTON_STEPS:
        return res
    P = kb.lift_plane(cam, s["x"], s["y"], s["h"])
    b = P / kb.norm(P)[:, None]
    root_err, angle = 0.0, 0.0
    for i, (t, ts, r) in enumerate(zip(th, s["ref"], s["r"])):
        if r == 0 or fp_mp(k, ts) < 0.1:
            continue
        root_err = max(root_err, float(abs(mp.mpf(float(t)) - ts) * fp_mp(k, ts) / (EPS * max(ts, mp.mpf(float(r))))))
        # the 50-digit bearing of the point (x, y) itself: its exact radius, the root moved there by Newton steps in 50 digits
        xe, ye = mp.mpf(float(s["x"][i])), mp.mpf(float(s["y"][i]))
        re_ = mp.sqrt(xe * xe + ye * ye)
        te = ts
        for _ in range(4):
            te = te - (f_mp(k, te) - re_) / fp_mp(k, te)
        e = (mp.sin(te) * xe / re_, mp.sin(te) * ye / re_, mp.cos(te))
        g = [mp.mpf(float(v)) for v in b[i]]
        cross = (g[1] * e[2] - g[2] * e[1], g[2] * e[0] - g[0] * e[2], g[0] * e[1] - g[1] * e[0])
        angle = max(angle, float(mp.atan2(mp.sqrt(sum(c * c for c in cross)), sum(p * q for p, q in zip(g, e))) / EPS))
    return res, root_err, angle


def test_specification_against_50_digits(sweep):
    need = 0
    for name, s in sweep.items():
        assert all(t is not None for t in s["ref"]), name  # the whole sweep lies on the monotone range: the reference finds a root
        res, root_err, angle = measure(s)
        steps = next(n for n in range(40) if measure(s, n) <= BAR_RESIDUAL)
        need = max(need, steps)
        print(f"{name}: {len(s['r'])} points, residual {res:.3f} eps r, root {root_err:.3f} eps, bearing {angle:.3f} eps, steps needed {steps}")
        assert res <= BAR_RESIDUAL and root_err <= BAR_ROOT and angle <= BAR_ANGLE, name
    assert sweep["RSFISH"]["within"] and len(sweep["RSFISH"]["r"]) == 329
    assert kb.NEWTON_STEPS == need + 2, need
    # beyond r_lim the reference's filter finds nothing, and the specification took the fallback: theta = r
    cam, h = kb.RSFISH, sweep["RSFISH"]["h"]
    r = np.linspace(float(h["r_lim"]) * 1.0001, 1.75, 12)
    assert all(reference_root(cam, v) is None for v in r)
    assert kb.fell_back(cam, r, h).all() and np.array_equal(kb.root(cam, r, h=h), r)


def test_sincos_against_50_digits():
    q = [np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi]
    th = np.concatenate([np.linspace(0.0, np.pi, 10 ** 4 - 12), q, [np.nextafter(v, 0.0) for v in q], [np.nextafter(v, 4.0) for v in q]])
    th = th[th <= np.pi + 1e-15]
    s, c = kb.sincos(th)
    es = max(ulps(mp.sin(mp.mpf(float(t))), a) for t, a in zip(th, s) if a != 0)
    ec = max(ulps(mp.cos(mp.mpf(float(t))), a) for t, a in zip(th, c))
    print(f"sin {es:.3f} ulp, cos {ec:.3f} ulp over {len(th)} points of [0, pi]")
    assert es <= BAR_SINCOS and ec <= BAR_SINCOS
    assert s[0] == 0.0 and c[0] == 1.0 and not np.signbit(s[0])


# ---- 3
def test_lift_gives_the_ray_back():
    rng = np.random.default_rng(5)
    for name, cam in kb.CAMERAS.items():
        W, H = kb.SIZES[name]
        rays = kb.cone(rng, 3000, cam, (W, H))
        px = kb.project(cam, rays)
        assert px[:, 0].min() > 0 and px[:, 0].max() < W - 1 and px[:, 1].min() > 0 and px[:, 1].max() < H - 1
        x, y = (px[:, 0] - cam["cx"]) / cam["fx"], (px[:, 1] - cam["cy"]) / cam["fy"]
        P = kb.lift_plane(cam, x, y)
        err = np.abs(P / kb.norm(P)[:, None] - rays).max()
        print(f"{name}: lift(project(ray)) - ray over the image: {err:.3e}")
        assert err <= 1e-9, name
        assert np.allclose(kb.norm(kb.bearings(cam, px.astype(np.float32))), 1.0, rtol=0, atol=4e-16)


# ---- 4
def test_branches(sweep):
    r = np.concatenate([np.linspace(0.0, np.pi, 1001), [1e-300, 3.2, 1e6, INF]])
    assert np.array_equal(bits(kb.root(kb.KB_IDEAL, r)), bits(r))  # all four zero: theta == r exactly (:771-774)
    assert np.array_equal(bits(kb.root(kb.KB_IDEAL, r, steps=1)), bits(r))  # ... after the first step already
    for name in ("KB_K5_0", "KB_K45_0"):
        res, _, angle = measure(sweep[name])
        assert res <= BAR_RESIDUAL and angle <= BAR_ANGLE, name
    assert kb.host_constants(kb.KB_K5_0)["theta_lim"] < np.pi  # (CLA without k5 turns down inside [0, pi])


# ---- 5
def test_checks(lib):
    cases = [(cam, 40) for cam in kb.CAMERAS.values()]
    cases += [(dict(kb.TUM, model=m), 40) for m in (1, 4, 7, -1)] + [(dict(cr.EUROC, model=m), 40) for m in (1, 4, 7, -1)]
    refused_fields = 0
    for base in (kb.TUM, kb.RSFISH):
        for key in kb.CHECKED:
            cases += [(dict(base, **{key: v}), 40) for v in (NAN, INF, -INF)]
            refused_fields += 3
        cases += [(dict(base, fx=0.0), 40), (dict(base, fy=0.0), 40), (dict(base, fx=-0.0), 40), (dict(base, fx=-190.9), 40)]
        cases += [(base, N) for N in (-1, 0, 7, 8, 4096, 4097)]
    refused = 0
    for cam, N in cases:
        want = kb.common_check(cam, N)
        why = lib.kt_check(_p(vec18(cam)), N)
        assert (why is not None) == want, (cam, N, why)
        assert why is None or why.startswith(b"lfvio_track"), why
        refused += want
    assert refused == 8 + refused_fields + 2 * 3 + 2 * 2
    why = lib.kt_check(_p(vec18(dict(kb.TUM, model=4))), 40)
    assert all(n in why for n in (b"LFVIO_CAM_OCAM", b"LFVIO_CAM_PINHOLE", b"LFVIO_CAM_MEI", b"LFVIO_CAM_KANNALA_BRANDT"))
    assert not kb.common_check(dict(kb.TUM, fx=-190.9), 40) and kb.common_check(dict(kb.TUM, k4=NAN), 40)
    # the other models: NaN in every field they do not read (vec18), accepted, and the TrackCam members they had
    for cam in (tr.PAL, tr.SKEW):
        t = track_cam(lib, cam)
        inv = np.float64(1.0) / (np.float64(cam["c"]) - np.float64(cam["d"]) * np.float64(cam["e"]))
        want = np.array([cam["cx"], cam["cy"], cam["c"], cam["d"], cam["e"], inv, *cam["poly"]] + [0.0] * 13, np.float64)
        assert np.array_equal(bits(t), bits(want)) and lib.kt_check(_p(vec18(cam)), 40) is None
    for cam in (cr.EUROC, cr.MV3DM):
        h = cr.host_constants(cam)
        want = np.array([cam["cx"], cam["cy"], 0, 0, 0, 0, 0, 0, 0, 0, 0, h["inv11"], h["inv13"], h["inv22"], h["inv23"], cam["k1"], cam["k2"],
                         cam["p1"], cam["p2"], cam.get("xi", 0.0), cam["model"], float(h["no_distortion"]), 0, 0], np.float64)
        assert np.array_equal(bits(track_cam(lib, cam)), bits(want)) and lib.kt_check(_p(vec18(cam)), 40) is None


# ---- 6
def test_restatement_reproduces_its_fixture(fx):
    rec = gen_kb.build()
    assert sorted(rec) == sorted(fx)
    for k in rec:
        a, b = np.asarray(rec[k]), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)), k
    assert list(fx["names"]) == list(kb.CASES) and sorted(len(fx[f"{n}/cur"]) for n in kb.CASES) == [7, 8] + [40] * 6


def test_fixture_cases_meet_c1_c2_and_none_drops(fx):
    n, cams = 0, set()
    for name in kb.CASES:
        cam, cur, forw, samples = kb.make_case(name)
        W, H = kb.SIZES[kb.CASES[name][0]]
        assert cur.min() >= 0 and forw.min() >= 0 and max(cur[:, 0].max(), forw[:, 0].max()) <= W - 1 and max(cur[:, 1].max(), forw[:, 1].max()) <= H - 1
        r = kb.reject(cam, cur, forw, samples)
        assert r["status"] == int(fx[f"{name}/status"])
        if r["status"] == 0:
            assert kb.conditions(r), (name, r["c1_gap"], r["c2_margin"])  # no case drops
            if len(cur) >= 30:
                assert 8 <= r["mask"].sum() < len(cur), name  # something is rejected
            n += 1
            cams.add(kb.CASES[name][0])
    assert n >= 7 and cams == set(kb.CAMERAS) and int(fx["cla_7/status"]) == 2
    for s in fx["sequences"]:
        ids = [fx[f"{s}/{j}/ids"] for j in range(int(fx[f"{s}/calls"]))]
        assert len(ids) == 4 and len(ids[0]) == 40
        assert any((i == -1).any() for i in ids) and any(len(set(i.tolist())) < len(i) for i in ids)
        v = [fx[f"{s}/{j}/velocity_3d"] for j in range(len(ids))]
        assert not v[0].any() and all(x.any() for x in v[1:])
        assert all(np.isfinite(fx[f"{s}/{j}/un_pts"]).all() for j in range(len(ids)))
