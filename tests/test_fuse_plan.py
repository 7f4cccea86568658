"""CPU tests of lf-vio_amd/csrc/fuse_plan.h — the plain C++ behind lfvio_cloud_fuse — compiled alone with g++ -ffp-contract=off -Wall
-Werror behind a ctypes shim and held to tests/fuse_ref.py.

  1  fuse_point is bit for bit the numpy text: index, (float)r and the reason of 20 000 seeded points through the three poses at
     960 x 480 and 8192 x 4096, with and without a range gate; the fractional pixel (fuse_equirect) as bytes; the special points (a
     NaN's sign is compared as a mask); CAMERA for one camera of each model at 64 x 48, points behind the camera included; the
     recorded cases of tests/golden/fuse_cases.npz
  2  every field layout: point_step 12, 16, 22 (unaligned) and 48 with the offsets permuted, both byte orders, by whole dwords where
     the layout allows it and byte by byte always, against fuse_ref.fields and the points packed
  3  every refusal of include/lfvio.h once, each beside its neighbour that is accepted; fuse_ref.check agrees on every one
  4  the launch geometry: a lane per point, 256 to a workgroup"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fuse_ref as fr
import project_ref as pr
from test_camera_project import inv20
from test_kb_ref import same_but_nan, vec18

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

SRC = r'''
#include "fuse_plan.h"
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
// pose: R[9], T[3], min_range, max_range.  ints: kind, width, height
static LfvioFuseIn in_of(const double *pose, const int *ints, const LfvioProjector *p) {
  LfvioFuseIn in = {};
  for (int i = 0; i < 9; i++) in.R[i] = pose[i];
  for (int i = 0; i < 3; i++) in.T[i] = pose[9 + i];
  in.min_range = pose[12], in.max_range = pose[13];
  in.kind = ints[0], in.width = ints[1], in.height = ints[2], in.proj = p;
  in.point_step = 12, in.off_y = 4, in.off_z = 8;
  return in;
}
extern "C" void fp_points(const double *pose, const int *ints, const double *cam, const double *inv, int n, const float *xyz, int *index, float *range, int *why) {
  const LfvioCamera k = cam_of(cam);
  const LfvioProjector p = proj_of(&k, inv);
  const LfvioFuseIn in = in_of(pose, ints, &p);
  const FuseView v = fuse_view(in);
  for (int i = 0; i < n; i++) {
    const FuseHit h = fuse_point(v, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    index[i] = h.index, range[i] = h.range, why[i] = h.why;
  }
}
extern "C" void fp_frac(int width, int height, int n, const double *P, double *f) {
  for (int i = 0; i < n; i++) {
    const double X = P[3 * i], Y = P[3 * i + 1], Z = P[3 * i + 2];
    const FuseFrac q = fuse_equirect(width, height, X, Y, Z, sqrt(X * X + Y * Y));
    f[2 * i] = q.fx, f[2 * i + 1] = q.fy;
  }
}
// data must be 4-aligned where the layout is read by dwords
extern "C" int fp_read(int step, int ox, int oy, int oz, int big, int force_bytes, int n, const unsigned char *data, float *xyz) {
  LfvioFuseIn in = {};
  in.point_step = step, in.off_x = ox, in.off_y = oy, in.off_z = oz, in.big_endian = big;
  FuseLayout l = fuse_layout(in);
  const int dwords = l.dwords;
  if (force_bytes) l.dwords = 0;
  for (int i = 0; i < n; i++) {
    const FuseXYZ p = fuse_read(l, data, (size_t)i);
    xyz[3 * i] = p.x, xyz[3 * i + 1] = p.y, xyz[3 * i + 2] = p.z;
  }
  return dwords;
}
// ints: n, point_step, off_x, off_y, off_z, big_endian, kind, width, height, image_mode, encoding, step, src_width, src_height
// nulls: bit 0 in, 1 out, 2 cloud, 3 proj, 4 camera, 5 fmt, 6 pixels.  wants: bit 0 colour, bit 1 image_out
extern "C" const char *fp_check(const int *ints, const double *pose, const double *cam, const double *inv, int nulls, int wants) {
  const LfvioCamera k = cam_of(cam);
  const LfvioProjector p = proj_of(nulls & 16 ? nullptr : &k, inv);
  unsigned char byte = 0;
  const LfvioImageFormat f = {ints[10], ints[11]};
  LfvioFuseIn in = {};
  in.cloud = nulls & 4 ? nullptr : &byte;
  in.n = ints[0], in.point_step = ints[1], in.off_x = ints[2], in.off_y = ints[3], in.off_z = ints[4], in.big_endian = ints[5];
  for (int i = 0; i < 9; i++) in.R[i] = pose[i];
  for (int i = 0; i < 3; i++) in.T[i] = pose[9 + i];
  in.min_range = pose[12], in.max_range = pose[13];
  in.kind = ints[6], in.width = ints[7], in.height = ints[8], in.proj = nulls & 8 ? nullptr : &p;
  in.image_mode = ints[9], in.fmt = nulls & 32 ? nullptr : &f, in.src_width = ints[12], in.src_height = ints[13];
  in.pixels = nulls & 64 ? nullptr : &byte;
  LfvioFuseOut out = {};
  out.colour = wants & 1 ? &byte : nullptr, out.image_out = wants & 2 ? &byte : nullptr;
  return fuse_check(nulls & 1 ? nullptr : &in, nulls & 2 ? nullptr : &out);
}
extern "C" void fp_consts(int *out) {
  out[0] = FUSE_MAX_POINTS, out[1] = FUSE_MIN_STEP, out[2] = FUSE_MAX_STEP, out[3] = FUSE_THREADS, out[4] = LFVIO_FUSE_EQUIRECT, out[5] = LFVIO_FUSE_CAMERA;
  out[6] = LFVIO_FUSE_IMAGE_NONE, out[7] = LFVIO_FUSE_IMAGE_GIVEN, out[8] = LFVIO_FUSE_IMAGE_REMAP, out[9] = FUSE_KEPT, out[10] = FUSE_GATE;
  out[11] = FUSE_PROJECTION, out[12] = (int)FUSE_INF_BITS, out[13] = (int)sizeof(LfvioFuseIn), out[14] = (int)sizeof(LfvioFuseOut);
  out[15] = (int)fuse_blocks(0), out[16] = (int)fuse_blocks(1), out[17] = (int)fuse_blocks(256), out[18] = (int)fuse_blocks(257), out[19] = (int)fuse_blocks(1 << 20);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="fuse_plan_")
    src, so = os.path.join(d, "fp.cpp"), os.path.join(d, "libfp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    dp, fp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    i = C.c_int
    so.fp_points.restype, so.fp_points.argtypes = None, [dp, ip, dp, dp, i, fp, ip, fp, ip]
    so.fp_frac.restype, so.fp_frac.argtypes = None, [i, i, i, dp, dp]
    so.fp_read.restype, so.fp_read.argtypes = i, [i, i, i, i, i, i, i, up, fp]
    so.fp_check.restype, so.fp_check.argtypes = C.c_char_p, [ip, dp, dp, dp, i, i]
    so.fp_consts.restype, so.fp_consts.argtypes = None, [ip]
    return so


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    return {k: z[k] for k in z.files}


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


PAL = pr.CAMS["PAL"][0]


def pose14(v):
    return np.concatenate([v["R"], v["T"], [v["min_range"], v["max_range"]]]).astype(np.float64)


def c_points(lib, v, P):
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    cam = v["cam"] or PAL
    n = len(P)
    index, rng, why = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    lib.fp_points(_p(pose14(v)), _p(np.array([v["kind"], v["width"], v["height"]], np.int32), C.c_int), _p(vec18(cam)), _p(inv20(cam)), n, _p(P, C.c_float),
                  _p(index, C.c_int), _p(rng, C.c_float), _p(why, C.c_int))
    return index, rng, why


def points_hold(lib, v, P, tag):
    gi, gr, gw = c_points(lib, v, P)
    wi, wr, ww = fr.points(v, P[:, 0], P[:, 1], P[:, 2])
    assert np.array_equal(gi, wi) and np.array_equal(gw, ww) and same_but_nan(gr, wr), tag
    return wi, ww


# ---- 1
def test_fuse_point_equirect(lib):
    P = fr.sphere_cloud(20000)
    sp = fr.special_cloud()
    for name, R, T in fr.poses():
        for W, H in ((960, 480), (8192, 4096), (33, 17)):
            for gate in ((0.0, INF), (5.0, 60.0)):
                v = fr.view(width=W, height=H, R=R, T=T, min_range=gate[0], max_range=gate[1])
                wi, ww = points_hold(lib, v, P, (name, W, H, gate))
                assert (ww == fr.KEPT).sum() > 5000 and ((ww == fr.GATE).sum() > 5000) == (gate[0] > 0.0)
                _, sw = points_hold(lib, v, sp, (name, W, H, gate, "special"))
                assert set(sw.tolist()) == {fr.KEPT, fr.GATE, fr.PROJECTION} or name != "identity" or gate[0] > 0.0
        # the fractional pixel itself, as bytes
        X, Y, Z = fr.transform(R, T, P[:, 0], P[:, 1], P[:, 2])
        Q = np.ascontiguousarray(np.stack([X, Y, Z], axis=1))
        got = np.zeros((len(Q), 2))
        lib.fp_frac(8192, 4096, len(Q), _p(Q), _p(got))
        wx, wy = fr.equirect_frac(8192, 4096, X, Y, Z)
        assert got[:, 0].tobytes() == wx.tobytes() and got[:, 1].tobytes() == wy.tobytes(), name


@pytest.mark.parametrize("name", ["PAL", "EUROC", "MV3DM", "TUM"])
def test_fuse_point_camera(lib, name):
    cam = pr.small(pr.CAMS[name][0], pr.CAMS[name][1][0] / 64)
    P = np.concatenate([fr.camera_cloud(name, 4000), fr.special_cloud()])
    for pname, R, T in fr.poses()[:2]:
        v = fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, R=R, T=T, cam=cam, min_range=0.2, max_range=25.0)
        wi, ww = points_hold(lib, v, P, (name, pname))
        assert (ww == fr.KEPT).sum() > 100 and (ww == fr.PROJECTION).sum() > 100 and (ww == fr.GATE).sum() > 10, (name, pname)
    if pr.model_of(cam) in (pr.CAM_PINHOLE, pr.CAM_MEI):
        # a point and its mirror image through the centre: the projection alone would take both
        Q = np.array([[0.1, -0.05, 2.0], [-0.1, 0.05, -2.0]], np.float32)
        half = dict(cam, xi=0.5) if pr.model_of(cam) == pr.CAM_MEI else cam  # (with xi >= 1 a MEI camera sees every direction but -z)
        wi, ww = points_hold(lib, fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=half), Q, name)
        assert wi[0] >= 0 and ww.tolist() == [fr.KEPT, fr.PROJECTION]


def test_recorded_cases(lib, fx):
    P = fx["P"]
    for name in fx["poses"]:
        v = fr.view(width=33, height=17, R=fx[f"{name}/R"], T=fx[f"{name}/T"], min_range=0.5, max_range=100.0)
        gi, gr, gw = c_points(lib, v, P)
        assert np.array_equal(gi, fx[f"{name}/index"]) and np.array_equal(gw, fx[f"{name}/why"]), name
        assert fr.range_image(gi, gr, 33, 17).tobytes() == fx[f"{name}/range"].tobytes(), name
    for name in fx["cams"]:
        v = fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=pr.cam_from_vector(fx[f"{name}/cam"]))
        gi, gr, gw = c_points(lib, v, fx[f"{name}/P"])
        assert np.array_equal(gi, fx[f"{name}/index"]) and np.array_equal(gw, fx[f"{name}/why"]) and (gi >= 0).sum() > 50, name
        assert fr.range_image(gi, gr, 64, 48).tobytes() == fx[f"{name}/range"].tobytes(), name


# ---- 2
LAYOUTS = ((12, (0, 4, 8)), (12, (8, 0, 4)), (16, (4, 8, 12)), (16, (12, 0, 8)), (22, (2, 6, 10)), (22, (18, 1, 9)), (22, (0, 4, 8)), (48, (0, 4, 8)),
           (48, (44, 16, 0)), (48, (5, 21, 33)), (13, (9, 0, 4)))


def test_field_layouts(lib):
    P = np.concatenate([fr.sphere_cloud(300, seed=5), fr.special_cloud()])
    n = len(P)
    for step, offs in LAYOUTS:
        for big in (0, 1):
            data = fr.pack_cloud(P, step, offs, big_endian=big, seed=step)
            want = np.stack(fr.fields(data, n, step, *offs, big), axis=1)
            assert same_but_nan(want, P) and want.view(np.uint32).tobytes() == P.view(np.uint32).tobytes()
            aligned = np.zeros(len(data) + 8, np.uint8)
            buf = aligned[(-aligned.ctypes.data) % 4:][:len(data)]
            buf[:] = data
            assert buf.ctypes.data % 4 == 0
            for force in (0, 1):
                got = np.zeros((n, 3), np.float32)
                dwords = lib.fp_read(step, *offs, big, force, n, _p(buf, C.c_ubyte), _p(got, C.c_float))
                assert dwords == int(step % 4 == 0 and all(o % 4 == 0 for o in offs)), (step, offs)
                assert got.view(np.uint32).tobytes() == P.view(np.uint32).tobytes(), (step, offs, big, force)


# ---- 3
def refused(lib, nulls=0, **kw):
    a = dict(n=5, point_step=16, offs=(0, 4, 8), big_endian=0, R=np.eye(3), T=(0.0, 0.0, 0.0), min_range=0.0, max_range=INF, kind=fr.FUSE_EQUIRECT, width=33,
             height=17, cam=PAL, image_mode=fr.IMAGE_NONE, encoding=2, step=0, src_width=64, src_height=48, want_colour=False, want_image=False)
    a.update(kw)
    cam = a["cam"]
    inv = inv20(cam) if "inv" not in a else np.asarray(a.pop("inv"), np.float64)
    ints = np.array([a["n"], a["point_step"], *a["offs"], a["big_endian"], a["kind"], a["width"], a["height"], a["image_mode"], a["encoding"], a["step"],
                     a["src_width"], a["src_height"]], np.int32)
    pose = np.concatenate([np.asarray(a["R"], np.float64).reshape(9), np.asarray(a["T"], np.float64), [a["min_range"], a["max_range"]]])
    got = lib.fp_check(_p(ints, C.c_int), _p(pose), _p(vec18(cam)), _p(inv), nulls, int(a["want_colour"]) | 2 * int(a["want_image"])) is not None
    if not nulls:
        if pr.model_of(cam) == 0:
            a["cam"] = dict(cam, inv_poly=tuple(inv))
        assert got == fr.check(**a), kw
    return got


def test_refusals_and_their_neighbours(lib):
    c = np.zeros(20, np.int32)
    lib.fp_consts(_p(c, C.c_int))
    assert c.tolist()[:13] == [1 << 20, 12, 1024, 256, 0, 1, 0, 1, 2, 0, 1, 2, 0x7f800000]
    assert np.array([0x7f800000], np.uint32).view(np.float32)[0] == np.inf
    from lfvio import abi
    assert c[13] == C.sizeof(abi.FuseInC) and c[14] == C.sizeof(abi.FuseOutC)
    assert not refused(lib)
    # null pointers where a count says they are read
    assert refused(lib, nulls=1) and refused(lib, nulls=2) and refused(lib, nulls=4) and not refused(lib, nulls=4, n=0)
    assert not refused(lib, nulls=8) and not refused(lib, nulls=16)  # (EQUIRECT reads no projector)
    assert refused(lib, nulls=8, kind=fr.FUSE_CAMERA) and refused(lib, nulls=16, kind=fr.FUSE_CAMERA) and not refused(lib, kind=fr.FUSE_CAMERA)
    for n, ok in ((-1, False), (0, True), (1 << 20, True), ((1 << 20) + 1, False)):
        assert refused(lib, n=n) != ok
    for step, ok in ((11, False), (12, True), (13, True), (1024, True), (1025, False), (0, False), (-12, False)):
        assert refused(lib, point_step=step) != ok
    for offs, ok in (((0, 4, 8), True), ((12, 4, 8), True), ((13, 4, 8), False), ((-1, 4, 8), False), ((0, 3, 8), False), ((0, 4, 7), False), ((0, 4, 4), False),
                     ((5, 9, 1), True), ((0, 4, 13), False), ((0, 12, 8), True), ((3, 12, 8), True), ((8, 0, 11), False)):
        assert refused(lib, offs=offs) != ok, offs
    for big, ok in ((0, True), (1, True), (2, False), (-1, False)):
        assert refused(lib, big_endian=big) != ok
    for k in range(9):
        for bad in (NAN, INF, -INF):
            R = np.eye(3).reshape(9)
            R[k] = bad
            assert refused(lib, R=R)
    for k in range(3):
        for bad in (NAN, INF):
            T = np.zeros(3)
            T[k] = bad
            assert refused(lib, T=T)
    for lo, hi, ok in ((0.0, INF, True), (0.0, 0.0, True), (2.0, 2.0, True), (-0.1, 5.0, False), (NAN, 5.0, False), (INF, INF, False), (2.0, 1.9, False),
                       (2.0, NAN, False), (2.0, -INF, False)):
        assert refused(lib, min_range=lo, max_range=hi) != ok, (lo, hi)
    for kind, ok in ((-1, False), (0, True), (1, True), (2, False)):
        assert refused(lib, kind=kind) != ok
    for side, ok in ((15, False), (16, True), (8192, True), (8193, False), (0, False)):
        assert refused(lib, width=side) != ok and refused(lib, height=side) != ok
    # CAMERA: a projector lfvio_cam_project refuses
    bad = pr.inv_poly_of(PAL)
    bad[3] = NAN
    assert refused(lib, kind=fr.FUSE_CAMERA, inv=bad) and not refused(lib, inv=bad)
    euroc = pr.CAMS["EUROC"][0]
    assert not refused(lib, kind=fr.FUSE_CAMERA, cam=euroc) and refused(lib, kind=fr.FUSE_CAMERA, cam=dict(euroc, fx=0.0))
    assert refused(lib, kind=fr.FUSE_CAMERA, cam=dict(euroc, model=1)) and not refused(lib, cam=dict(euroc, model=1))
    # the image
    for mode, ok in ((-1, False), (0, True), (1, True), (2, True), (3, False)):
        assert refused(lib, image_mode=mode) != ok
    assert refused(lib, want_colour=True) and refused(lib, want_image=True)
    for mode in (fr.IMAGE_GIVEN, fr.IMAGE_REMAP):
        assert not refused(lib, image_mode=mode, want_colour=True, want_image=True)
        assert refused(lib, image_mode=mode, nulls=64) and not refused(lib, image_mode=mode, nulls=32)  # null pixels; a null format is mono8
        for enc, ok in ((-1, False), (0, True), (1, False), (2, True), (7, True), (8, False)):
            assert refused(lib, image_mode=mode, encoding=enc) != ok
        row = (33 if mode == fr.IMAGE_GIVEN else 64) * 3
        for step, ok in ((-1, False), (0, True), (row - 1, False), (row, True), (row + 5, True), (65536, True), (65537, False)):
            assert refused(lib, image_mode=mode, step=step) != ok, (mode, step)
    for side, ok in ((15, False), (16, True), (8192, True), (8193, False)):
        assert refused(lib, image_mode=fr.IMAGE_REMAP, src_width=side, encoding=0) != ok and refused(lib, image_mode=fr.IMAGE_REMAP, src_height=side) != ok
        assert not refused(lib, image_mode=fr.IMAGE_GIVEN, src_width=side) and not refused(lib, src_height=side)  # (only REMAP reads them)


# ---- 4
def test_launch_geometry(lib):
    c = np.zeros(20, np.int32)
    lib.fp_consts(_p(c, C.c_int))
    assert c[15:20].tolist() == [0, 1, 1, 2, 4096]
