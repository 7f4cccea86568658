"""lfvio_cloud_fuse on the device against the numpy text (tests/fuse_ref.py), as bytes.

  1  index, range and counts: n in {0, 1, 63, 64, 65, 1000, 4097}; EQUIRECT at 16 x 16, 33 x 17, 37 x 16 and once at 960 x 480 through
     the three poses; CAMERA for one camera of each model at 64 x 48 (and a MEI with xi < 1), points behind the camera included; the
     recorded cases of tests/golden/fuse_cases.npz
  2  layouts: point_step 12, 16, 22 (unaligned), 48 and 13 with the offsets permuted, in both byte orders
  3  special points: zeros, NaN and +-inf coordinates, both range gates hit exactly, the seam and the poles; 500 points on ONE pixel
     at distinct ranges (the minimum wins whatever the order); the same cloud shuffled gives the same range bytes
  4  images through mono8, bgr8, bgra8, mono16 and bgr8 with a padded step.  GIVEN on seeded noise: colour is the unpainted bytes even
     where another point paints that pixel, image_out with and without paint_on.  REMAP from a 64 x 48 source through a 33 x 17 map:
     image_out equals fuse_ref applied to project_ref.remap's output, and a following lfvio_remap_apply of the same and of another
     source geometry is still right
  5  state and refusals: every refusal leaves every output byte untouched; REMAP before any build, after lfvio_remap_reset and with a
     resident map of another size is refused; NULL outputs in every combination
  6  three lfvio_track_frame frames give the same bytes with lfvio_cloud_fuse calls interleaved as without"""
import itertools
import os

import numpy as np
import pytest

import fuse_ref as fr
import project_ref as pr
from lfvio import abi
from test_fuse_plan import LAYOUTS

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ERR_ARG = -1  # LFVIO_ERR_ARG
ENC = dict(mono8=abi.IMG_MONO8, bgr8=abi.IMG_BGR8, bgra8=abi.IMG_BGRA8, mono16=abi.IMG_MONO16)
FORMATS = (("mono8", 0), ("bgr8", 0), ("bgra8", 0), ("mono16", 0), ("bgr8", 8))  # (encoding, bytes of padding behind a row)
SIZES = (0, 1, 63, 64, 65, 1000, 4097)
ALL = ("index", "range", "colour", "image_out", "counts")
PAINT = (255, 0, 0, 77)

_cloud = {}


def cloud():
    if "P" not in _cloud:
        _cloud["P"] = fr.sphere_cloud(4097, seed=9, hi=60.0)
    return _cloud["P"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    return {k: z[k] for k in z.files}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def call(eng, v, P, point_step=12, offs=(0, 4, 8), big=0, **kw):
    P = np.asarray(P, np.float32).reshape(-1, 3)
    data = fr.pack_cloud(P, point_step, offs, big_endian=big, seed=len(P))
    return eng.cloud_fuse(data, len(P), point_step, offs, v["width"], v["height"], kind=v["kind"], big_endian=big, R=v["R"], T=v["T"], min_range=v["min_range"],
                          max_range=v["max_range"], cam=v["cam"], **kw)


def holds(eng, v, P, tag, **kw):
    P = np.asarray(P, np.float32).reshape(-1, 3)
    got = call(eng, v, P, **kw)
    want = fr.fuse(v, P[:, 0], P[:, 1], P[:, 2])
    for key in ("index", "range", "counts"):
        assert same(got[key], want[key]), (tag, key)
    return want


# ---- 1
@pytest.mark.parametrize("W,H", [(16, 16), (33, 17), (37, 16)])
def test_equirect(eng, W, H):
    P = cloud()
    for name, R, T in fr.poses():
        for n in SIZES:
            want = holds(eng, fr.view(width=W, height=H, R=R, T=T, min_range=1.0, max_range=50.0), P[:n], (name, n))
        assert want["counts"][fr.KEPT] > 2000 and want["counts"][fr.GATE] > 300 and np.isfinite(want["range"]).sum() > W * H // 2


def test_equirect_at_the_nodes_size(eng):
    want = holds(eng, fr.view(width=960, height=480, R=fr.node_R(), T=fr.NODE_T), cloud(), "960 x 480")
    assert want["counts"].tolist() == [4097, 0, 0] and 3900 < np.isfinite(want["range"]).sum() <= 4097


@pytest.mark.parametrize("name", ["PAL", "EUROC", "MV3DM", "MV3DM_HALF", "TUM"])
def test_camera(eng, name):
    base = name.split("_")[0]
    cam = pr.small(pr.CAMS[base][0], pr.CAMS[base][1][0] / 64)
    if name == "MV3DM_HALF":
        cam = dict(cam, xi=0.5)  # (with xi >= 1 a MEI camera sees every direction but -z)
    P = fr.camera_cloud(base, 4097)
    for n in SIZES:
        want = holds(eng, fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=cam, min_range=0.2, max_range=25.0), P[:n], (name, n))
    assert want["counts"][fr.KEPT] > 200 and want["counts"][fr.GATE] > 10
    assert want["counts"][fr.PROJECTION] > (1000 if name in ("EUROC", "MV3DM_HALF") else 100)  # behind the camera
    holds(eng, fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=cam, R=fr.node_R(), T=fr.NODE_T), np.concatenate([P[:500], fr.special_cloud()]), name)


def test_recorded_cases(eng, fx):
    for name in fx["poses"]:
        v = fr.view(width=33, height=17, R=fx[f"{name}/R"], T=fx[f"{name}/T"], min_range=0.5, max_range=100.0)
        got = call(eng, v, fx["P"])
        assert same(got["index"], fx[f"{name}/index"]) and same(got["range"], fx[f"{name}/range"]), name
        assert got["counts"].tolist() == [(fx[f"{name}/why"] == k).sum() for k in range(3)], name
    for name in fx["cams"]:
        v = fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=pr.cam_from_vector(fx[f"{name}/cam"]))
        got = call(eng, v, fx[f"{name}/P"])
        assert same(got["index"], fx[f"{name}/index"]) and same(got["range"], fx[f"{name}/range"]), name


# ---- 2
def test_layouts(eng):
    P = np.concatenate([cloud()[:1000], fr.special_cloud()])
    v = fr.view(width=33, height=17, R=fr.random_R(), T=(0.3, -0.2, 0.1), min_range=1.0, max_range=50.0)
    assert {s for s, _ in LAYOUTS} >= {12, 16, 22, 48}
    for step, offs in LAYOUTS:
        for big in (0, 1):
            holds(eng, v, P, (step, offs, big), point_step=step, offs=offs, big=big)


# ---- 3
def test_special_points(eng):
    sp = fr.special_cloud()
    for name, R, T in fr.poses():
        for W, H in ((16, 16), (33, 17), (960, 480)):
            want = holds(eng, fr.view(width=W, height=H, R=R, T=T), sp, (name, W, H))
    i = fr.points(fr.view(width=960, height=480), sp[:, 0], sp[:, 1], sp[:, 2])
    assert {fr.KEPT, fr.GATE, fr.PROJECTION} == set(i[2].tolist()) and (i[2][-9:] == fr.GATE).all() and i[2][0] == fr.GATE  # NaN, +-inf; zeros
    # both range gates hit exactly: r = 5, 10, 2.5 in one direction
    P = np.array([[0.0, 3.0, 4.0], [0.0, 6.0, 8.0], [0.0, 1.5, 2.0]], np.float32)
    for lo, hi, kept in ((5.0, 10.0, 2), (np.nextafter(5.0, 6.0), 10.0, 1), (5.0, np.nextafter(10.0, 0.0), 1), (2.5, 2.5, 1), (0.0, INF, 3), (0.0, 0.0, 0)):
        want = holds(eng, fr.view(width=33, height=17, min_range=lo, max_range=hi), P, (lo, hi))
        assert want["counts"][fr.KEPT] == kept


def test_many_points_on_one_pixel(eng):
    d = np.array([0.3, 0.8, 0.2]) / np.linalg.norm([0.3, 0.8, 0.2])
    r = np.random.default_rng(410).permutation(np.linspace(2.0, 40.0, 500))
    P = (d[None, :] * r[:, None]).astype(np.float32)
    v = fr.view(width=33, height=17)
    want = holds(eng, v, P, "one pixel")
    assert len(set(want["index"].tolist())) == 1 and want["index"][0] >= 0 and len(set(np.linalg.norm(P.astype(np.float64), axis=1).astype(np.float32))) == 500
    pixel = want["range"].reshape(-1)[want["index"][0]]
    assert np.isinf(want["range"]).sum() == 33 * 17 - 1 and abs(pixel - 2.0) < 1e-5
    for order in (np.argsort(r), np.argsort(-r)):
        assert same(call(eng, v, P[order])["range"], want["range"])
    # a whole cloud shuffled: the same range bytes
    Q = cloud()
    v = fr.view(width=33, height=17, R=fr.node_R(), T=fr.NODE_T)
    first = holds(eng, v, Q, "in order")["range"]
    assert same(call(eng, v, Q[np.random.default_rng(411).permutation(len(Q))])["range"], first)


# ---- 4
def noise(seed, W, H, fmt):
    name, pad = fmt
    enc = ENC[name]
    bpp = pr.BPP[enc]
    step = W * bpp + pad if pad else 0
    img = pr.noise_image(seed, W, H, enc, step)
    return img, enc, step, bpp, np.ascontiguousarray(img[:, :W * bpp])


@pytest.mark.parametrize("fmt", FORMATS)
def test_given_image(eng, fmt):
    for k, (W, H) in enumerate(((33, 17), (37, 16), (64, 48))):
        img, enc, step, bpp, rows = noise(200 + k, W, H, fmt)
        P = cloud()[:1500]
        v = fr.view(width=W, height=H, R=fr.random_R(), T=(0.3, -0.2, 0.1), min_range=1.0, max_range=50.0)
        for paint in (None, PAINT):
            want = fr.fuse(v, P[:, 0], P[:, 1], P[:, 2], image=rows, bpp=bpp, paint=paint)
            got = call(eng, v, P, image=img, encoding=enc, step=step, paint=paint, want=ALL)
            for key in ALL:
                assert same(got[key], want[key]), (fmt, W, H, paint, key)
        # several points share most pixels: colour is the unpainted image everywhere, and the paint is in the image
        index = want["index"]
        assert len(set(index[index >= 0].tolist())) < (index >= 0).sum() and same(want["colour"][index >= 0], rows.reshape(-1, bpp)[index[index >= 0]])
        assert not same(want["image_out"], rows) and (want["image_out"].reshape(-1, bpp)[index[index >= 0]] == np.array(PAINT[:bpp], np.uint8)).all()
        assert same(call(eng, v, P, image=img, encoding=enc, step=step, want=("image_out",))["image_out"], rows)
    # a null format is mono8
    img, enc, step, bpp, rows = noise(210, 33, 17, ("mono8", 0))
    v = fr.view(width=33, height=17)
    got = call(eng, v, cloud()[:100], image=img, paint=PAINT, want=ALL)
    assert same(got["image_out"], fr.fuse(v, *cloud()[:100].T, image=rows, bpp=1, paint=PAINT)["image_out"])


def test_remap_image(eng):
    W, H, sw, sh = 33, 17, 64, 48
    cam = pr.small(pr.CAMS["PAL"][0], 20.0)
    mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
    P = cloud()[:1500]
    v = fr.view(width=W, height=H, R=fr.node_R(), T=fr.NODE_T, min_range=1.0, max_range=50.0)
    for k, fmt in enumerate(FORMATS):
        src, enc, step, bpp, _ = noise(220 + k, sw, sh, fmt)
        flat = pr.remap(src, mx, my, sw, sh, enc, step)
        assert flat.any()
        for paint, want_names in ((PAINT, ALL), (None, ALL), (PAINT, ("image_out",)), (PAINT, ("colour", "counts"))):
            want = fr.fuse(v, P[:, 0], P[:, 1], P[:, 2], image=flat, bpp=bpp, paint=paint)
            got = call(eng, v, P, image=src, image_mode=abi.FUSE_IMAGE_REMAP, src_size=(sw, sh), encoding=enc, step=step, paint=paint, want=want_names)
            for key in want_names:
                assert same(got[key], want[key]), (fmt, paint, key)
        # a following lfvio_remap_apply of the same and of another source geometry is still right, and the fused call after it
        assert same(eng.remap_apply(src, sw, sh, (W, H), encoding=enc, step=step), flat), fmt
        other, oenc, ostep, _, _ = noise(230 + k, 128, 48, ("bgra8", 0))
        assert same(eng.remap_apply(other, 128, 48, (W, H), encoding=oenc, step=ostep), pr.remap(other, mx, my, 128, 48, oenc, ostep)), fmt
        got = call(eng, v, P, image=src, image_mode=abi.FUSE_IMAGE_REMAP, src_size=(sw, sh), encoding=enc, step=step, want=("image_out",))
        assert same(got["image_out"], flat), fmt
    eng.remap_reset()


# ---- 5
def test_state_and_refusals(eng):
    W, H, sw, sh = 33, 17, 64, 48
    P = cloud()[:100]
    v = fr.view(width=W, height=H)
    img, enc, step, bpp, rows = noise(240, W, H, ("bgr8", 0))
    src = noise(241, sw, sh, ("bgr8", 0))[0]
    data = fr.pack_cloud(P, 16, (0, 4, 8))

    def keep():
        return dict(index=np.full(100, -7, np.int32), range=np.full((H, W), -3.0, np.float32), colour=np.full((100, 3), 201, np.uint8),
                    image_out=np.full((H, W * 3), 202, np.uint8), counts=np.full(3, -9, np.int32))

    def refused(tag, **kw):
        a = dict(cloud=data, n=100, point_step=16, offs=(0, 4, 8), width=W, height=H, image=img, encoding=enc, step=step, paint=PAINT)
        a.update(kw)
        before = keep()
        rc, out = eng.cloud_fuse(a.pop("cloud"), a.pop("n"), a.pop("point_step"), a.pop("offs"), a.pop("width"), a.pop("height"), out=keep(), want=(), check=False, **a)
        assert rc == ERR_ARG, tag
        for key in ALL:
            assert same(out[key], before[key]), (tag, key)

    eng.remap_reset()
    remap_kw = dict(image=src, image_mode=abi.FUSE_IMAGE_REMAP, src_size=(sw, sh))
    refused("REMAP before any build", **remap_kw)
    cam = pr.small(pr.CAMS["PAL"][0], 20.0)
    mx, my = eng.remap_build(cam, abi.MAP_EQUIRECT, W, H)
    flat = pr.remap(src, mx, my, sw, sh, enc, 0)
    ok = eng.cloud_fuse(data, 100, 16, (0, 4, 8), W, H, encoding=enc, want=ALL, **remap_kw)
    assert same(ok["image_out"], flat) and same(ok["index"], fr.points(v, *P.T)[0])
    refused("REMAP through a map of another size", width=37, **remap_kw)
    bad_R, bad_T = np.eye(3), np.zeros(3)
    bad_R[1, 2], bad_T[0] = NAN, INF
    bad_inv = list(pr.inv_poly_of(cam))
    bad_inv[2] = NAN
    for tag, kw in (("null cloud", dict(cloud=None)), ("n < 0", dict(n=-1)), ("n too large", dict(n=(1 << 20) + 1)), ("step 11", dict(point_step=11)),
                    ("step 1025", dict(point_step=1025)), ("offset past the point", dict(offs=(0, 4, 13))), ("negative offset", dict(offs=(-1, 4, 8))),
                    ("fields overlap", dict(offs=(0, 3, 8))), ("big_endian 2", dict(big_endian=2)), ("NaN in R", dict(R=bad_R)), ("inf in T", dict(T=bad_T)),
                    ("min_range < 0", dict(min_range=-1.0)), ("min_range NaN", dict(min_range=NAN)), ("max < min", dict(min_range=2.0, max_range=1.0)),
                    ("max NaN", dict(max_range=NAN)), ("kind 2", dict(kind=2)), ("width 15", dict(width=15)), ("height 8193", dict(height=8193)),
                    ("CAMERA without a projector", dict(kind=abi.FUSE_CAMERA)), ("a bad inverse polynomial", dict(kind=abi.FUSE_CAMERA, cam=dict(cam, inv_poly=bad_inv))),
                    ("fy == 0", dict(kind=abi.FUSE_CAMERA, cam=dict(pr.CAMS["EUROC"][0], fy=0.0))), ("image_mode 3", dict(image_mode=3)),
                    ("null pixels", dict(image=None, image_mode=abi.FUSE_IMAGE_GIVEN)), ("encoding 1", dict(encoding=1)), ("step below a row", dict(step=W * 3 - 1)),
                    ("step above 65536", dict(step=65537)), ("src_width 15", dict(remap_kw, src_size=(15, sh))), ("src_height 8193", dict(remap_kw, src_size=(sw, 8193))),
                    ("colour and image_out without an image", dict(image=None))):
        refused(tag, **kw)
        # the resident maps and their integer map still serve the next lfvio_remap_apply
        assert same(eng.remap_apply(src, sw, sh, (W, H), encoding=enc), flat), tag
    # NULL outputs in every combination
    want = fr.fuse(v, *P.T, image=rows, bpp=bpp, paint=PAINT)
    for r in range(len(ALL) + 1):
        for names in itertools.combinations(ALL, r):
            got = eng.cloud_fuse(data, 100, 16, (0, 4, 8), W, H, image=img, encoding=enc, paint=PAINT, want=names)
            assert set(got) == set(names)
            for key in names:
                assert same(got[key], want[key]), (names, key)
    # without an image: index, range and counts in every combination
    for r in range(4):
        for names in itertools.combinations(("index", "range", "counts"), r):
            got = eng.cloud_fuse(data, 100, 16, (0, 4, 8), W, H, want=names)
            for key in names:
                assert same(got[key], want[key]), (names, key)
    eng.remap_reset()
    refused("REMAP after lfvio_remap_reset", **remap_kw)


# ---- 6
def test_track_frames_do_not_see_the_fusion(eng):
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
    src = noise(250, 64, 48, ("bgr8", 0))[0]
    given = noise(251, 64, 48, ("mono8", 0))[0]
    P = cloud()[:1000]

    def between(k):
        if k % 2 == 0:
            eng.remap_build(pal, abi.MAP_EQUIRECT, 33, 17, want_maps=False)
        call(eng, fr.view(width=33, height=17), P, image=src, image_mode=abi.FUSE_IMAGE_REMAP, src_size=(64, 48), encoding=abi.IMG_BGR8, paint=PAINT, want=ALL)
        call(eng, fr.view(kind=fr.FUSE_CAMERA, width=64, height=48, cam=pr.small(pr.CAMS["TUM"][0], 8.0)), P, point_step=22, offs=(2, 6, 10), image=given, want=ALL)

    mixed = run(between)
    assert S == 100 and len(plain) == 3
    for a, b in zip(plain, mixed):
        assert a["num_points"] > 0
        for key in TABLE:
            assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), key
        for key in ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject"):
            assert a[key] == b[key], key
        for key, val in a["stages"].items():
            w = b["stages"][key]
            assert (val is None and w is None) or np.array_equal(np.asarray(val), np.asarray(w)), key
    eng.remap_reset()
