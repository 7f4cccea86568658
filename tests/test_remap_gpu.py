"""lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply / lfvio_remap_reset on the device against the numpy text
(tests/project_ref.py), as bytes: NaN positions as a mask (x86 and gfx950 make NaNs of opposite sign), every other value bit for bit.

  1  cam_project: n in {0, 1, 63, 64, 65, 1000} for one camera of each model (PAL, EUROC, MV3DM, TUM), the special rays, and the
     rays tests/golden/remap_cases.npz records for all 13 cameras
  2  remap_build: EQUIRECT on PAL, EUROC, MV3DM and TUM at 16 x 16, 33 x 17 (a multiple of no tile) and 960 x 480; PERSPECTIVE on PAL
     with the 90-degree view along -z; PERSPECTIVE on EUROC_ND with M = K^-1, which is the identity to the round-trip bar of
     tests/test_project_ref.py (5.1e-13 px: in float, exactly); the recorded small maps.  With map_x = map_y = NULL the resident map
     gives the same apply output
  3  remap_apply: 64 x 48 and 1280 x 960 seeded noise (every wrong index shows) as mono8, bgr8, bgra8, mono16 and bgr8 with a padded
     step, through maps 16, 33 and 37 wide (row bytes no multiple of 4 for 1, 2 and 3 bytes per pixel) and 960 x 480, against
     project_ref.remap; the recorded outputs of the fixture
  4  hand-made maps through the public route: PERSPECTIVE on an undistorted PINHOLE with fx = fy = 1, cx = cy = 0, so that the map IS
     the ray's (X / Z, Y / Z): columns k + 0.5 (ties to even), negative coordinates, exactly src_width - 0.5 (rounds to src_width:
     outside), far outside, +-inf and NaN from Z = 0; a map whose every entry is outside gives an all-zero image
  5  a second apply with another format or source size after one build is right (the integer map is rebuilt), and going back too
  6  state: apply before any build and after lfvio_remap_reset is refused and leaves `out` untouched; a refused build (every kind of
     refusal of tests/test_remap_plan.py once) leaves outputs untouched and the resident map serving the next apply
  7  three lfvio_track_frame frames give the same bytes with remap_build / remap_apply / cam_project calls interleaved as without"""
import ctypes as C
import os

import numpy as np
import pytest

import project_ref as pr
from lfvio import abi
from test_kb_ref import same_but_nan

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ERR_ARG = -1  # LFVIO_ERR_ARG
ENC = dict(mono8=abi.IMG_MONO8, bgr8=abi.IMG_BGR8, bgra8=abi.IMG_BGRA8, mono16=abi.IMG_MONO16)
FORMATS = (("mono8", 0), ("bgr8", 0), ("bgra8", 0), ("mono16", 0), ("bgr8", 8))  # (encoding, bytes of padding behind a row)
UNIT = dict(model=2, fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0)  # the map is the ray's (X / Z, Y / Z)


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "remap_cases.npz"))
    return {k: z[k] for k in z.files}


_maps = {}


def ref_map(name, kind, W, H, M=None, cam=None):
    """project_ref.build, computed once per case and shared."""
    key = (name, kind, W, H, None if M is None else np.asarray(M, np.float64).tobytes())
    if key not in _maps:
        _maps[key] = pr.build(cam or pr.CAMS[name][0], kind, W, H, M)
    return _maps[key]


def source(seed, sw, sh, fmt):
    name, pad = fmt
    enc = ENC[name]
    step = sw * pr.BPP[enc] + pad if pad else 0
    return pr.noise_image(seed, sw, sh, enc, step), enc, step


def apply_holds(eng, mx, my, sw, sh, fmt, seed, tag):
    src, enc, step = source(seed, sw, sh, fmt)
    H, W = mx.shape
    got = eng.remap_apply(src, sw, sh, (W, H), encoding=enc, step=step)
    want = pr.remap(src, mx, my, sw, sh, enc, step)
    assert got.shape == want.shape and np.array_equal(got, want), tag
    return got


# ---- 1
@pytest.mark.parametrize("name", ["PAL", "EUROC", "MV3DM", "TUM"])
def test_cam_project(eng, name):
    cam = pr.CAMS[name][0]
    rays = np.concatenate([pr.image_rays(name, 500), pr.sphere_rays(name, 500)])
    for n in (0, 1, 63, 64, 65, 1000):
        got = eng.cam_project(cam, rays[:n])
        assert got.shape == (n, 2) and same_but_nan(got, pr.project(cam, rays[:n])), (name, n)
    sp = pr.special_rays()
    want = pr.project(cam, sp)
    assert same_but_nan(eng.cam_project(cam, sp), want) and np.isnan(want).any() and not np.isnan(want).all()


def test_cam_project_on_the_fixture(eng, fx):
    for name in fx["names"]:
        cam = pr.cam_from_vector(fx[f"{name}/cam"])
        assert same_but_nan(eng.cam_project(cam, fx[f"{name}/P"]), fx[f"{name}/px"]), name


def test_cam_project_refusals(eng):
    pal, rays = pr.CAMS["PAL"][0], pr.sphere_rays("PAL", 8)
    keep = np.full((8, 2), -7.0)
    bad_inv = list(pr.inv_poly_of(pal))
    bad_inv[7] = NAN
    for cam, P, n in ((None, rays, 8), (dict(pal, inv_poly=bad_inv), rays, 8), (dict(pr.CAMS["EUROC"][0], fx=0.0), rays, 8), (pal, None, 8),
                      (pal, rays, -1), (pal, rays, (1 << 20) + 1)):
        rc, out = eng.cam_project(cam, P, out=keep.copy(), n=n, check=False)
        assert rc == ERR_ARG and np.array_equal(out, keep), (cam is None, n)


# ---- 2
@pytest.mark.parametrize("name", ["PAL", "EUROC", "MV3DM", "TUM"])
def test_build_equirect(eng, name):
    cam = pr.CAMS[name][0]
    for W, H in ((16, 16), (33, 17), (960, 480)):
        wx, wy = ref_map(name, pr.MAP_EQUIRECT, W, H)
        mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
        assert mx.shape == (H, W) and same_but_nan(mx, wx) and same_but_nan(my, wy), (name, W, H)


def test_build_perspective(eng):
    for W, H in ((16, 16), (33, 17), (960, 480)):
        M = pr.look_down_M(W, H)
        wx, wy = ref_map("PAL", pr.MAP_PERSPECTIVE, W, H, M)
        mx, my = eng.remap_build(pr.CAMS["PAL"][0], abi.MAP_PERSPECTIVE, W, H, M=M)
        assert same_but_nan(mx, wx) and same_but_nan(my, wy), (W, H)
        # M = K^-1 on a PINHOLE without distortion: the identity, to the measured round-trip bar
        nd = pr.CAMS["EUROC_ND"][0]
        mx, my = eng.remap_build(nd, abi.MAP_PERSPECTIVE, W, H, M=pr.K_inverse(nd))
        wx, wy = ref_map("EUROC_ND", pr.MAP_PERSPECTIVE, W, H, pr.K_inverse(nd))
        assert same_but_nan(mx, wx) and same_but_nan(my, wy), (W, H)
        i, j = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
        assert np.abs(mx - i).max() <= 5.1e-13 and np.abs(my - j).max() <= 5.1e-13, (W, H)


def test_build_recorded_maps_and_null_outputs(eng, fx):
    for m in fx["maps"]:
        cam = pr.cam_from_vector(fx[f"{m}/cam"])
        kind, (W, H), M = int(fx[f"{m}/kind"]), fx[f"{m}/size"].tolist(), fx[f"{m}/M"]
        mx, my = eng.remap_build(cam, kind, W, H, M=M)
        assert same_but_nan(mx, fx[f"{m}/x"]) and same_but_nan(my, fx[f"{m}/y"]), m
        first = {g: eng.remap_apply(fx[f"src_{g[0]}_{g[1]}"], pr.SRC_W, pr.SRC_H, (W, H), encoding=g[0], step=g[1]) for g in pr.GATHERS}
        for g, out in first.items():
            assert np.array_equal(out, fx[f"{m}/out_{g[0]}_{g[1]}"]), (m, g)
        eng.remap_reset()
        assert eng.remap_build(cam, kind, W, H, M=M, want_maps=False) is None  # map_x = map_y = NULL: the resident map alone
        for g, out in first.items():
            assert np.array_equal(eng.remap_apply(fx[f"src_{g[0]}_{g[1]}"], pr.SRC_W, pr.SRC_H, (W, H), encoding=g[0], step=g[1]), out), (m, g)


# ---- 3
@pytest.mark.parametrize("W,H", [(16, 16), (33, 17), (37, 16)])
def test_apply_small_outputs(eng, W, H):
    """Row bytes 16 .. 148: no multiple of 4 at 33 and 37 wide for 1, 2 and 3 bytes per pixel; 33 x 17 and 37 x 16 end in a tail."""
    for sw, sh, s in ((64, 48, 20.0), (1280, 960, 1.0)):
        cam = pr.small(pr.CAMS["PAL"][0], s)
        wx, wy = ref_map(f"PAL/{s}", pr.MAP_EQUIRECT, W, H, cam=cam)
        mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
        assert same_but_nan(mx, wx) and same_but_nan(my, wy)
        inside = pr.offsets(wx, wy, sw, sh, sw, 1) >= 0
        assert inside.any() and not inside.all()
        for k, fmt in enumerate(FORMATS):
            apply_holds(eng, wx, wy, sw, sh, fmt, 10 * k + sw, (W, H, sw, fmt))


def test_apply_the_nodes_shape(eng):
    """1280 x 960 -> 960 x 480, the reference node's shape, every format."""
    W, H, sw, sh = 960, 480, 1280, 960
    wx, wy = ref_map("PAL", pr.MAP_EQUIRECT, W, H)
    eng.remap_build(pr.CAMS["PAL"][0], abi.MAP_EQUIRECT, W, H, want_maps=False)
    for k, fmt in enumerate(FORMATS):
        out = apply_holds(eng, wx, wy, sw, sh, fmt, 50 + k, fmt)
        assert out.any()


# ---- 4
def test_hand_made_maps(eng):
    W, H, sw, sh = 37, 16, 64, 48
    # u = 2 i - 8.5: -8.5 .. 63.5 in steps of 2 (k + 0.5, negative, exactly sw - 0.5); v = 3 j - 4.5: -4.5 .. 40.5
    M = [[2.0, 0.0, -8.5], [0.0, 3.0, -4.5], [0.0, 0.0, 1.0]]
    mx, my = eng.remap_build(UNIT, abi.MAP_PERSPECTIVE, W, H, M=M)
    assert np.array_equal(mx[0], 2.0 * np.arange(W, dtype=np.float32) - 8.5) and np.array_equal(my[:, 0], 3.0 * np.arange(H, dtype=np.float32) - 4.5)
    sx = pr.remap_index(mx[0])
    assert sx[4] == 0 and sx[5] == 2 and sx[6] == 4 and sx[35] == 62 and sx[36] == 64 and mx[0, 36] == sw - 0.5  # -0.5 -> 0, 1.5 -> 2, 63.5 -> 64: outside
    for k, fmt in enumerate(FORMATS):
        out = apply_holds(eng, mx, my, sw, sh, fmt, 70 + k, fmt)
        bpp = pr.BPP[ENC[fmt[0]]]
        assert not out[:, 36 * bpp:].any() and not out[:, :4 * bpp].any() and not out[:2].any() and out[2:, 4 * bpp:36 * bpp].any()
    # far outside on both sides, and +-inf / NaN from Z = 0 on row 0 and column 0
    M = [[1e9, 0.0, 0.0], [0.0, -1e9, 5e9], [1.0, 1.0, 0.0]]
    mx, my = eng.remap_build(UNIT, abi.MAP_PERSPECTIVE, W, H, M=M)
    wx, wy = pr.build(UNIT, pr.MAP_PERSPECTIVE, W, H, M)
    assert same_but_nan(mx, wx) and same_but_nan(my, wy) and np.isnan(mx[0, 0]) and np.isinf(my[0, 0]) and np.abs(mx[3, 3]) > 1e8
    apply_holds(eng, wx, wy, sw, sh, ("bgr8", 0), 80, "far")
    # every entry outside: an all-zero image, whatever was in `out`
    for M in ([[0.0, 0.0, -100.0], [0.0, 0.0, -100.0], [0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], np.zeros((3, 3))):
        mx, my = eng.remap_build(UNIT, abi.MAP_PERSPECTIVE, W, H, M=M)
        assert (pr.offsets(mx, my, sw, sh, sw * 3, 3) < 0).all()
        src, enc, step = source(81, sw, sh, ("bgr8", 0))
        out = eng.remap_apply(src, sw, sh, (W, H), encoding=enc, out=np.full((H, W * 3), 255, np.uint8))
        assert not out.any()


# ---- 5
def test_apply_after_a_change_of_source(eng):
    W, H = 33, 17
    cams = {64: pr.small(pr.CAMS["PAL"][0], 20.0), 1280: pr.CAMS["PAL"][0]}
    wx, wy = ref_map("PAL/20.0", pr.MAP_EQUIRECT, W, H, cam=cams[64])
    eng.remap_build(cams[64], abi.MAP_EQUIRECT, W, H, want_maps=False)
    order = ((64, 48, ("bgr8", 0)), (64, 48, ("mono8", 0)), (64, 48, ("bgr8", 8)), (128, 48, ("bgr8", 0)), (64, 96, ("bgr8", 0)), (1280, 960, ("mono16", 0)),
             (64, 48, ("bgr8", 0)), (64, 48, ("bgr8", 0)))
    for k, (sw, sh, fmt) in enumerate(order):
        apply_holds(eng, wx, wy, sw, sh, fmt, 90 + k, (k, sw, sh, fmt))
    # a build after applies writes the integer map for the last source itself: the next apply of that source is right at once
    cam2 = pr.CAMS["TUM"][0]
    tx, ty = eng.remap_build(pr.small(cam2, 8.0), abi.MAP_EQUIRECT, W, H)
    apply_holds(eng, tx, ty, 64, 48, ("bgr8", 0), 99, "after a build")
    apply_holds(eng, tx, ty, 64, 48, ("bgra8", 0), 100, "after a build, another format")


# ---- 6
def test_state(eng):
    W, H, sw, sh = 33, 17, 64, 48
    src, enc, step = source(110, sw, sh, ("bgr8", 0))
    keep = np.full((H, W * 3), 201, np.uint8)
    eng.remap_reset()
    eng.klt_reset()
    w, h = C.c_int(0), C.c_int(0)
    no_image = eng.lib.lfvio_klt_level(eng.ctx, 0, C.byref(w), C.byref(h), None)  # what lfvio_klt_level returns with no resident image
    assert no_image == ERR_ARG
    for _ in range(2):
        rc, out = eng.remap_apply(src, sw, sh, (W, H), encoding=enc, out=keep.copy(), check=False)
        assert rc == no_image and np.array_equal(out, keep)
        cam = pr.small(pr.CAMS["PAL"][0], 20.0)
        mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
        want = apply_holds(eng, mx, my, sw, sh, ("bgr8", 0), 110, "built")
        # refused applies leave `out` alone
        for kw in (dict(rows=None), dict(src_width=15), dict(src_height=8193), dict(encoding=1), dict(step=191), dict(step=65537)):
            a = dict(rows=src, src_width=sw, src_height=sh, encoding=enc, step=step)
            a.update(kw)
            rc, out = eng.remap_apply(a["rows"], a["src_width"], a["src_height"], (W, H), encoding=a["encoding"], step=a["step"], out=keep.copy(), check=False)
            assert rc == ERR_ARG and np.array_equal(out, keep), kw
        # refused builds leave their outputs alone and the resident map serving the next apply
        bad_inv = list(pr.inv_poly_of(cam))
        bad_inv[0] = INF
        fkeep = np.full((H, W), -3.0, np.float32)
        for kw in (dict(cam=None), dict(cam=dict(cam, inv_poly=bad_inv)), dict(cam=dict(pr.CAMS["EUROC"][0], fy=NAN)), dict(kind=2), dict(kind=1, M=np.full(9, NAN)),
                   dict(width=15), dict(height=8193), dict(map_x=False), dict(map_y=False)):
            a = dict(cam=cam, kind=abi.MAP_EQUIRECT, width=W, height=H, M=None, map_x=fkeep.copy(), map_y=fkeep.copy())
            a.update(kw)
            rc, ox, oy = eng.remap_build(a["cam"], a["kind"], a["width"], a["height"], M=a["M"], map_x=a["map_x"], map_y=a["map_y"], check=False)
            assert rc == ERR_ARG, kw
            assert all(o is False or np.array_equal(o, fkeep) for o in (ox, oy)), kw
            assert np.array_equal(eng.remap_apply(src, sw, sh, (W, H), encoding=enc), want), kw
        eng.remap_reset()


# ---- 7
def test_track_frames_do_not_see_the_remap(eng):
    from test_track_frame import KW, S, TABLE, when, words
    from test_tracker_chain import CAM, frames

    imgs = frames()[:3]

    def run(between):
        eng.track_frame_reset()
        out = []
        for k, img in enumerate(imgs):
            between(k)
            out.append(eng.track_frame(img, when(k), CAM, words=words(k), stages=True, **KW))
            between(k + 10)
        return out

    plain = run(lambda k: None)
    pal = pr.small(pr.CAMS["PAL"][0], 20.0)
    src, enc, step = source(120, 64, 48, ("bgr8", 0))

    width = [0]

    def between(k):
        if k % 2 == 0:
            width[0] = 33 + k
            eng.remap_build(pal, abi.MAP_EQUIRECT, width[0], 17, want_maps=k == 0)
        eng.remap_apply(src, 64, 48, (width[0], 17), encoding=enc)
        eng.cam_project(pr.CAMS["TUM"][0], pr.sphere_rays("TUM", 65))

    mixed = run(between)
    assert S == 100 and len(plain) == 3
    for a, b in zip(plain, mixed):
        assert a["num_points"] > 0
        for key in TABLE:
            assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), key
        for key in ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject"):
            assert a[key] == b[key], key
        for key, v in a["stages"].items():
            w = b["stages"][key]
            assert (v is None and w is None) or np.array_equal(np.asarray(v), np.asarray(w)), key
    eng.remap_reset()
