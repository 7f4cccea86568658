"""CPU tests of lf-vio_amd/csrc/remap_plan.h — the plain C++ behind lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply — compiled
alone with g++ -ffp-contract=off -Wall -Werror behind a ctypes shim and held to tests/project_ref.py.

  1  every refusal of include/lfvio.h, each beside its neighbour that is accepted: null projector / camera / input, a camera
     track_camera_check refuses, a non-finite inv_poly entry (OCam) and M entry (PERSPECTIVE only), n outside [0, 1 << 20], null P or px
     with n > 0, output and source width and height outside [16, 8192], an encoding outside the table, a step below a row and above
     65536, exactly one of map_x / map_y null, an unknown kind; project_ref's checks agree on every one
  2  remap_index: every k + 0.5, k = -3 .. 3 (-0.5 and 0.5 give 0, 1.5 gives 2: ties to even), 32766.5, 32767.5, +-1e10, +-inf, NaN,
     -0.0, and 4096 seeded floats, against project_ref.remap_index; remap_offset against project_ref.offsets
  3  the map of every fixture case, entry by entry on the host (remap_entry), equals project_ref.build and the recorded maps as
     bytes, NaNs as a mask; the recorded outputs are project_ref.remap of the recorded sources
  4  the rebuild decision: the integer map is rebuilt exactly when there is none or the source's width, height, step or bytes per
     pixel differ; step 0 and step == width * bytes per pixel are the same geometry
  5  the launch geometry covers every pixel: 33 x 17 is 2 x 3 tiles; a run of n pixels takes ceil(ceil(n / 4) / 256) workgroups"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import project_ref as pr
from test_camera_project import inv20
from test_kb_ref import bits, same_but_nan, vec18

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

SRC = r'''
#include "remap_plan.h"
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
// nulls: bit 0 the projector, bit 1 its camera, bit 2 the input struct
extern "C" const char *rp_project_check(const double *cam, const double *inv, int nulls, int n, int have_P, int have_px) {
  const LfvioCamera k = cam_of(cam);
  const LfvioProjector p = proj_of(nulls & 2 ? nullptr : &k, inv);
  double x = 0.0;
  return remap_project_check(nulls & 1 ? nullptr : &p, n, have_P ? &x : nullptr, have_px ? &x : nullptr);
}
extern "C" const char *rp_build_check(const double *cam, const double *inv, int nulls, int kind, int width, int height, const double *M, int have_x, int have_y) {
  const LfvioCamera k = cam_of(cam);
  const LfvioProjector p = proj_of(nulls & 2 ? nullptr : &k, inv);
  LfvioRemapIn in;
  in.proj = nulls & 1 ? nullptr : &p, in.kind = kind, in.width = width, in.height = height;
  for (int i = 0; i < 9; i++) in.M[i] = M[i];
  float x = 0.0f;
  return remap_build_check(nulls & 4 ? nullptr : &in, have_x ? &x : nullptr, have_y ? &x : nullptr);
}
extern "C" const char *rp_apply_check(int null_fmt, int encoding, int step, int sw, int sh, int have_pixels, int have_out) {
  const LfvioImageFormat f = {encoding, step};
  unsigned char x = 0;
  return remap_apply_check(null_fmt ? nullptr : &f, sw, sh, have_pixels ? &x : nullptr, have_out ? &x : nullptr);
}
extern "C" void rp_index(int n, const float *v, int *out) {
  for (int i = 0; i < n; i++) out[i] = remap_index(v[i]);
}
extern "C" void rp_offset(int n, const float *mx, const float *my, int encoding, int step, int sw, int sh, int *out) {
  const LfvioImageFormat f = {encoding, step};
  const RemapGeom g = remap_geom(f, sw, sh);
  for (int i = 0; i < n; i++) out[i] = remap_offset(mx[i], my[i], g);
}
extern "C" void rp_map(const double *cam, const double *inv, int kind, int width, int height, const double *M, float *mx, float *my) {
  const LfvioCamera k = cam_of(cam);
  const ProjCam q = proj_cam(proj_of(&k, inv));
  for (int j = 0; j < height; j++)
    for (int i = 0; i < width; i++) {
      const RemapEntry e = remap_entry(q, kind, width, height, M, i, j);
      mx[(size_t)j * width + i] = e.x, my[(size_t)j * width + i] = e.y;
    }
}
// built: 0 no integer map, 1 one for (enc0, step0, sw0, sh0); the question: a source (enc1, step1, sw1, sh1)
extern "C" int rp_needs_index(int built, int enc0, int step0, int sw0, int sh0, int enc1, int step1, int sw1, int sh1) {
  RemapResident r;
  r.valid = true, r.width = 33, r.height = 17;
  const LfvioImageFormat f0 = {enc0, step0}, f1 = {enc1, step1};
  if (built) r.indexed = true, r.geom = remap_geom(f0, sw0, sh0);
  return remap_needs_index(r, remap_geom(f1, sw1, sh1));
}
extern "C" void rp_grid(int width, int height, unsigned *out) {
  const RemapGrid g = remap_build_grid(width, height);
  out[0] = g.x, out[1] = g.y, out[2] = remap_apply_blocks((size_t)width * height), out[3] = remap_project_blocks(width);
}
extern "C" void rp_consts(int *out) {
  out[0] = REMAP_MAX_POINTS, out[1] = REMAP_TILE_W, out[2] = REMAP_TILE_H, out[3] = REMAP_THREADS, out[4] = REMAP_RUN, out[5] = REMAP_PROJECT_THREADS;
  out[6] = LFVIO_MAP_EQUIRECT, out[7] = LFVIO_MAP_PERSPECTIVE, out[8] = LFVIO_OCAM_INV_POLY_SIZE, out[9] = (int)sizeof(LfvioProjector), out[10] = (int)sizeof(LfvioRemapIn);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="remap_plan_")
    src, so = os.path.join(d, "rp.cpp"), os.path.join(d, "librp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    i = C.c_int
    so.rp_project_check.restype, so.rp_project_check.argtypes = C.c_char_p, [dp, dp, i, i, i, i]
    so.rp_build_check.restype, so.rp_build_check.argtypes = C.c_char_p, [dp, dp, i, i, i, i, dp, i, i]
    so.rp_apply_check.restype, so.rp_apply_check.argtypes = C.c_char_p, [i] * 7
    so.rp_index.restype, so.rp_index.argtypes = None, [i, fp, ip]
    so.rp_offset.restype, so.rp_offset.argtypes = None, [i, fp, fp, i, i, i, i, ip]
    so.rp_map.restype, so.rp_map.argtypes = None, [dp, dp, i, i, i, dp, fp, fp]
    so.rp_needs_index.restype, so.rp_needs_index.argtypes = i, [i] * 9
    so.rp_grid.restype, so.rp_grid.argtypes = None, [i, i, C.POINTER(C.c_uint)]
    so.rp_consts.restype, so.rp_consts.argtypes = None, [ip]
    return so


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "remap_cases.npz"))
    return {k: z[k] for k in z.files}


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


PAL, EUROC, TUM = (pr.CAMS[n][0] for n in ("PAL", "EUROC", "TUM"))
EYE = np.eye(3).reshape(9)


def build_refused(lib, cam=PAL, inv=None, nulls=0, kind=0, width=33, height=17, M=EYE, have_x=1, have_y=1):
    inv = inv20(cam) if inv is None else np.asarray(inv, np.float64)
    M = np.ascontiguousarray(M, np.float64)
    got = lib.rp_build_check(_p(vec18(cam)), _p(inv), nulls, kind, width, height, _p(M), have_x, have_y) is not None
    if not nulls & 6:  # (the numpy text has no struct to be null)
        c = None if nulls & 1 else (dict(cam, inv_poly=tuple(inv)) if pr.model_of(cam) == 0 else cam)
        assert got == pr.build_check(c, kind, width, height, M, bool(have_x), bool(have_y))
    return got


def project_refused(lib, cam=PAL, inv=None, nulls=0, n=5, have_P=1, have_px=1):
    inv = inv20(cam) if inv is None else np.asarray(inv, np.float64)
    got = lib.rp_project_check(_p(vec18(cam)), _p(inv), nulls, n, have_P, have_px) is not None
    if not nulls and have_P and have_px:
        assert got == pr.project_check(dict(cam, inv_poly=tuple(inv)) if pr.model_of(cam) == 0 else cam, n)
    return got


def apply_refused(lib, null_fmt=0, encoding=2, step=0, sw=64, sh=48, have_pixels=1, have_out=1):
    got = lib.rp_apply_check(null_fmt, encoding, step, sw, sh, have_pixels, have_out) is not None
    if have_pixels and have_out:
        assert got == pr.apply_check(0 if null_fmt else encoding, 0 if null_fmt else step, sw, sh)
    return got


# ---- 1
def test_refusals_and_their_neighbours(lib):
    c = np.zeros(11, np.int32)
    lib.rp_consts(_p(c, C.c_int))
    assert c.tolist()[:9] == [1 << 20, 32, 8, 256, 4, 64, 0, 1, 20] and c[9] == 8 + 20 * 8 and c[10] == 8 + 16 + 72
    # lfvio_remap_build
    assert not build_refused(lib)
    for nulls in (1, 2, 4):
        assert build_refused(lib, nulls=nulls)
    for cam in (EUROC, TUM, pr.CAMS["MV3DM"][0]):
        assert not build_refused(lib, cam=cam)
        assert build_refused(lib, cam=dict(cam, fx=NAN)) and build_refused(lib, cam=dict(cam, fy=0.0)) and build_refused(lib, cam=dict(cam, model=1))
    bad = pr.inv_poly_of(PAL)
    bad[19] = INF
    assert build_refused(lib, inv=bad) and not build_refused(lib, cam=EUROC, inv=bad)  # (only OCam reads inv_poly)
    for kind, ok in ((-1, False), (0, True), (1, True), (2, False)):
        assert build_refused(lib, kind=kind) != ok
    for k in range(9):
        for v in (NAN, INF):
            M = EYE.copy()
            M[k] = v
            assert build_refused(lib, kind=1, M=M) and not build_refused(lib, kind=0, M=M)  # (EQUIRECT does not read M)
    for side, ok in ((15, False), (16, True), (8192, True), (8193, False), (0, False), (-16, False)):
        assert build_refused(lib, width=side) != ok and build_refused(lib, height=side) != ok
    assert build_refused(lib, have_x=0) and build_refused(lib, have_y=0) and not build_refused(lib, have_x=0, have_y=0)
    # lfvio_cam_project
    assert not project_refused(lib)
    assert project_refused(lib, nulls=1) and project_refused(lib, nulls=2) and project_refused(lib, inv=bad) and project_refused(lib, cam=dict(TUM, k3=NAN))
    for n, ok in ((-1, False), (0, True), (1, True), (1 << 20, True), ((1 << 20) + 1, False)):
        assert project_refused(lib, n=n) != ok
    assert project_refused(lib, have_P=0) and project_refused(lib, have_px=0) and not project_refused(lib, n=0, have_P=0, have_px=0)
    # lfvio_remap_apply
    assert not apply_refused(lib) and not apply_refused(lib, null_fmt=1)
    assert apply_refused(lib, have_pixels=0) and apply_refused(lib, have_out=0)
    for side, ok in ((15, False), (16, True), (8192, True), (8193, False)):
        assert apply_refused(lib, sw=side, encoding=0) != ok and apply_refused(lib, sh=side) != ok
    for enc, ok in ((-1, False), (0, True), (1, False), (2, True), (3, True), (4, True), (5, True), (6, True), (7, True), (8, False)):
        assert apply_refused(lib, encoding=enc) != ok
    for step, ok in ((-1, False), (0, True), (191, False), (192, True), (200, True), (65536, True), (65537, False)):
        assert apply_refused(lib, step=step) != ok  # bgr8, 64 wide: a row is 192 bytes


# ---- 2
def test_remap_index(lib):
    v = np.array([k + 0.5 for k in range(-3, 4)] + [32766.5, 32767.5, 1e10, -1e10, INF, -INF, NAN, -0.0, 32767.0, -32768.0, -32768.5, -32769.5, 0.49999997],
                 np.float32)
    got = np.zeros(len(v), np.int32)
    lib.rp_index(len(v), _p(v, C.c_float), _p(got, C.c_int))
    assert got.tolist() == [-2, -2, 0, 0, 2, 2, 4, 32766, 32767, 32767, -32768, 32767, -32768, -32768, 0, 32767, -32768, -32768, -32768, 0]
    assert np.array_equal(got, pr.remap_index(v))
    rng = np.random.default_rng(311)
    w = np.concatenate([rng.uniform(-70000.0, 70000.0, 2048), rng.integers(-40, 1300, 2048) + 0.5]).astype(np.float32)
    got = np.zeros(len(w), np.int32)
    lib.rp_index(len(w), _p(w, C.c_float), _p(got, C.c_int))
    assert np.array_equal(got, pr.remap_index(w))
    # the integer map's entry: inside exactly for 0 <= sx < sw and 0 <= sy < sh
    mx = np.array([-0.5, 0.5, 62.5, 63.49, 63.5, 5.0, 5.0, 5.0, 5.0, NAN, 5.0, 1e10], np.float32)
    my = np.array([0.0, 0.0, 47.0, 47.0, 47.0, -0.51, -0.5, 47.5, 47.51, 3.0, NAN, 3.0], np.float32)
    for enc, step in pr.GATHERS + ((7, 130),):
        got = np.zeros(len(mx), np.int32)
        lib.rp_offset(len(mx), _p(mx, C.c_float), _p(my, C.c_float), enc, step, 64, 48, _p(got, C.c_int))
        bpp, st = pr.BPP[enc], step or 64 * pr.BPP[enc]
        assert got.tolist() == [0, 0, 47 * st + 62 * bpp, 47 * st + 63 * bpp, -1, -1, 5 * bpp, -1, -1, -1, -1, -1], (enc, step)
        assert np.array_equal(got, pr.offsets(mx, my, 64, 48, st, bpp))


# ---- 3
def c_map(lib, cam, kind, W, H, M):
    mx, my = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    M = np.zeros(9) if M is None else np.ascontiguousarray(M, np.float64).reshape(9)
    lib.rp_map(_p(vec18(cam)), _p(inv20(cam)), kind, W, H, _p(M), _p(mx, C.c_float), _p(my, C.c_float))
    return mx, my


def test_maps_of_the_fixture(lib, fx):
    assert list(fx["maps"]) == list(pr.MAPS)
    inside = {}
    for m in fx["maps"]:
        cam = pr.cam_from_vector(fx[f"{m}/cam"])
        kind, (W, H), M = int(fx[f"{m}/kind"]), fx[f"{m}/size"].tolist(), fx[f"{m}/M"]
        mx, my = c_map(lib, cam, kind, W, H, M)
        wx, wy = pr.build(cam, kind, W, H, M)
        for got, want, rec in ((mx, wx, fx[f"{m}/x"]), (my, wy, fx[f"{m}/y"])):
            assert same_but_nan(got, want) and same_but_nan(want, rec), m
        for enc, step in pr.GATHERS:
            src = fx[f"src_{enc}_{step}"]
            want = pr.remap(src, wx, wy, pr.SRC_W, pr.SRC_H, enc, step)
            assert np.array_equal(want, fx[f"{m}/out_{enc}_{step}"]) and want.shape == (H, W * pr.BPP[enc]), (m, enc, step)
        inside[m] = float((pr.offsets(wx, wy, pr.SRC_W, pr.SRC_H, pr.SRC_W, 1) >= 0).mean())
    # every map has pixels inside and (but the identity) outside the source: both sides of the border are in the fixture
    assert inside.pop("euroc_nd_identity_37x16") == 1.0 and all(0.2 < v < 0.9 for v in inside.values()), inside
    # the identity: M = K^-1 on a PINHOLE without distortion gives map_x = i, map_y = j
    ident = fx["euroc_nd_identity_37x16/x"], fx["euroc_nd_identity_37x16/y"]
    assert np.array_equal(ident[0], np.tile(np.arange(37, dtype=np.float32), (16, 1)))
    assert np.array_equal(ident[1], np.tile(np.arange(16, dtype=np.float32)[:, None], (1, 37)))
    assert np.isnan(fx["euroc_equirect_16x16/x"]).any()  # Z == 0 on the row of the horizon: a NaN entry is outside


# ---- 4
def test_rebuild_decision(lib):
    q = lambda built, a, b: bool(lib.rp_needs_index(built, *a, *b))
    bgr = (2, 0, 1280, 960)
    assert q(0, bgr, bgr) and not q(1, bgr, bgr)
    assert not q(1, bgr, (2, 3840, 1280, 960)) and not q(1, bgr, (3, 0, 1280, 960))  # step 0 is width * 3; rgb8 is 3 bytes too
    for other in ((2, 3844, 1280, 960), (2, 0, 1279, 960), (2, 0, 1280, 961), (0, 0, 1280, 960), (4, 0, 1280, 960), (6, 0, 1280, 960)):
        assert q(1, bgr, other) and q(1, other, bgr), other
        f = lambda g: (g[2], g[3], g[1] or g[2] * pr.BPP[g[0]], pr.BPP[g[0]])
        assert pr.needs_rebuild(f(bgr), f(other)) and not pr.needs_rebuild(f(other), f(other)) and pr.needs_rebuild(None, f(other))


# ---- 5
def test_launch_geometry(lib):
    g = np.zeros(4, np.uint32)
    for (W, H), want in (((33, 17), (2, 3)), ((16, 16), (1, 2)), ((960, 480), (30, 60)), ((8192, 8192), (256, 1024))):
        lib.rp_grid(W, H, _p(g, C.c_uint))
        n = W * H
        assert (int(g[0]), int(g[1])) == want and int(g[0]) * 32 >= W and int(g[1]) * 8 >= H
        assert int(g[2]) == -(-(-(-n // 4)) // 256) and int(g[2]) * 256 * 4 >= n and int(g[3]) == -(-W // 64)
