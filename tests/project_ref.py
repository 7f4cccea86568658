"""numpy specification of the projections and of the remap (include/lfvio.h: lfvio_cam_project, lfvio_remap_build, lfvio_remap_apply;
DESIGN.md 3w): spaceToPlane of the four camera models, the two ray generators, the float map, the index of a map entry and the nearest
remap, one rounding per operation.  lf-vio_amd/csrc/camera_atan.h, camera_models.h (cam_project) and remap_plan.h are the same text in
C++ for the host and the device; they are held to this file bit for bit (tests/test_camera_project.py, tests/test_remap_plan.py,
tests/test_remap_gpu.py), and this file to a 50-digit evaluation of the reference's definitions (tests/test_project_ref.py).

  atan               fdlibm's s_atan.c scheme in + - * /, comparisons and fabs
  project            OCAMCamera / PinholeCamera / CataCamera / EquidistantCamera::spaceToPlane, chosen by the camera's model
  equirect_rays      GetremapMat's ray of every output pixel (pointcloud_image_fusion.cpp:83-114)
  perspective_rays   initUndistortRectifyMap's ray M (u, v, 1) (ScaramuzzaCamera.cc:723-777), M supplied by the caller
  build              (map_x, map_y) float32 [height, width]
  remap_index        saturate_cast<short>: round to nearest even, clamp to [-32768, 32767]; a NaN: -32768
  offsets            the integer map: byte offset of the source pixel, or -1
  remap              cv::remap(..., INTER_NEAREST), BORDER_CONSTANT 0, on `bpp`-byte pixels
  build_check, apply_check, project_check   the argument checks of remap_plan.h; True: refused

A camera is a dict as in track_ref / camera_ref / kb_ref; an OCam camera carries `inv_poly` (up to 20 numbers) for the projection."""
import numpy as np

import camera_ref as cr
import kb_ref as kb
import track_ref as tr
from lfvio import synth

F64 = np.float64
CAM_OCAM, CAM_PINHOLE, CAM_MEI, CAM_KANNALA_BRANDT = 0, 2, 3, 5
INV_POLY_SIZE = 20
MAP_EQUIRECT, MAP_PERSPECTIVE = 0, 1
MIN_SIDE, MAX_SIDE, MAX_POINTS, MAX_STEP = 16, 8192, 1 << 20, 65536
BPP = {0: 1, 2: 3, 3: 3, 4: 4, 5: 4, 6: 2, 7: 2}

PAL = dict(tr.PAL, inv_poly=synth.OCAM_INV)
SKEW = dict(tr.SKEW, inv_poly=synth.OCAM_INV)

# ---- the arctangent: atanhi / atanlo and aT[0 .. 10] of s_atan.c, fdlibm 5.3 (Sun Microsystems, 1993; public)
ATANHI = tuple(F64(v) for v in (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00))
ATANLO = tuple(F64(v) for v in (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17))
AT = tuple(F64(v) for v in (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                            9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                            4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02))
ATAN_EDGES = (0.4375, 0.6875, 1.1875, 2.4375)
ATAN_TINY, ATAN_HUGE = F64(2.0) ** -29, F64(2.0) ** 66


def _pick(i0, i1, i2, i3, v3, v2, v1, v0, below):
    return np.where(i3, v3, np.where(i2, v2, np.where(i1, v1, np.where(i0, v0, below))))


def atan(x):
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        i0, i1, i2, i3 = (a >= e for e in ATAN_EDGES)
        num = _pick(i0, i1, i2, i3, F64(-1.0), a - F64(1.5), a - F64(1.0), F64(2.0) * a - F64(1.0), a)
        den = _pick(i0, i1, i2, i3, a, F64(1.0) + F64(1.5) * a, a + F64(1.0), F64(2.0) + a, F64(1.0))
        hi = _pick(i0, i1, i2, i3, ATANHI[3], ATANHI[2], ATANHI[1], ATANHI[0], ATANHI[0])
        lo = _pick(i0, i1, i2, i3, ATANLO[3], ATANLO[2], ATANLO[1], ATANLO[0], ATANLO[0])
        t = num / den
        z = t * t
        w = z * z
        s1 = z * (AT[0] + w * (AT[2] + w * (AT[4] + w * (AT[6] + w * (AT[8] + w * AT[10])))))
        s2 = w * (AT[1] + w * (AT[3] + w * (AT[5] + w * (AT[7] + w * AT[9]))))
        ts = t * (s1 + s2)
        r = np.where(i0, hi - ((ts - lo) - t), t - ts)
        r = np.where(a >= ATAN_HUGE, ATANHI[3] + ATANLO[3], r)
        r = np.where(x < 0.0, -r, r)
        return np.where(a < ATAN_TINY, x, r)


# ---- the projections
PI_HI, PI_LO, PIO2 = F64(3.14159265358979311600e+00), F64(1.22464679914735317723e-16), F64(1.57079632679489655800e+00)


def model_of(cam):
    return cam.get("model", CAM_OCAM)


def inv_poly_of(cam):
    v = np.zeros(INV_POLY_SIZE)
    p = np.asarray(cam["inv_poly"], F64)
    v[:len(p)] = p
    return v


def no_distortion(cam):
    return cr.host_constants(cam)["no_distortion"]


def kb_theta(rxy, Z):
    """The angle in [0, pi] with tangent rxy / Z.  Z > 0: atan(q); Z < 0: pi + atan(q); Z == 0: pi / 2 off the axis; otherwise q (a NaN)."""
    q = rxy / Z
    a = atan(q)
    return np.where(Z > 0.0, a, np.where(Z < 0.0, PI_HI + (a + PI_LO), np.where((Z == 0.0) & (rxy > 0.0), PIO2, q)))


def project(cam, P):
    """P [..., 3] float64 -> (u, v) [..., 2] float64."""
    P = np.asarray(P, F64)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    m = model_of(cam)
    with np.errstate(all="ignore"):
        if m == CAM_OCAM:
            c, d, e, cx, cy = (F64(cam[k]) for k in ("c", "d", "e", "cx", "cy"))
            n = np.sqrt(X * X + Y * Y)
            theta = atan(-Z / n)
            rho, t = np.zeros_like(theta), np.ones_like(theta)
            for coef in inv_poly_of(cam):
                rho = rho + t * coef
                t = t * theta
            inv = F64(1.0) / n
            xn, yn = (X * inv) * rho, (Y * inv) * rho
            return np.stack([(xn * c + yn * d) + cx, (xn * e + yn) + cy], axis=-1)
        fx, fy, cx, cy = (F64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        if m == CAM_KANNALA_BRANDT:
            rxy = np.sqrt(X * X + Y * Y)
            theta = kb_theta(rxy, Z)
            tiny = rxy < 1e-10
            cphi, sphi = np.where(tiny, F64(1.0), X / rxy), np.where(tiny, F64(0.0), Y / rxy)
            r = kb.f_poly(kb.ks(cam), theta)
            return np.stack([fx * (r * cphi) + cx, fy * (r * sphi) + cy], axis=-1)
        z = Z if m == CAM_PINHOLE else Z + F64(cam["xi"]) * tr.norm(P)
        x, y = X / z, Y / z
        if not no_distortion(cam):
            dx, dy = cr._dist(cam, x, y)  # the text the lift uses, as cam_project uses cam_distortion
            x, y = x + dx, y + dy
        return np.stack([fx * x + cx, fy * y + cy], axis=-1)


# ---- the rays of a map
PI, TWO_PI = F64(np.pi), F64(2.0) * F64(np.pi)


def equirect_rays(width, height):
    """[height, width, 3]: lon = ((double)i / width - 0.5) (2 pi), lat = -(((double)j / height - 0.5) pi), sine and cosine by kb_ref.sincos."""
    i, j = np.arange(width, dtype=F64)[None, :], np.arange(height, dtype=F64)[:, None]
    lon = (i / F64(width) - F64(0.5)) * TWO_PI
    lat = -((j / F64(height) - F64(0.5)) * PI)
    slon, clon = kb.sincos(lon)
    slat, clat = kb.sincos(lat)
    return np.stack(np.broadcast_arrays(clat * slon, clat * clon, slat), axis=-1)


def perspective_rays(width, height, M):
    """[height, width, 3]: row r of M gives (M[r][0] i + M[r][1] j) + M[r][2]."""
    M = np.asarray(M, F64).reshape(3, 3)
    i, j = np.arange(width, dtype=F64)[None, :], np.arange(height, dtype=F64)[:, None]
    with np.errstate(all="ignore"):
        return np.stack([(M[r, 0] * i + M[r, 1] * j) + M[r, 2] for r in range(3)], axis=-1)


def build(cam, kind, width, height, M=None):
    rays = equirect_rays(width, height) if kind == MAP_EQUIRECT else perspective_rays(width, height, M)
    with np.errstate(all="ignore"):
        uv = project(cam, rays)
        return uv[..., 0].astype(np.float32), uv[..., 1].astype(np.float32)


# ---- the gather
def remap_index(v):
    """saturate_cast<short>(float): rint (ties to even), clamped; NaN -> -32768 (outside every image)."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        r = np.rint(v)
        r = np.where(r >= np.float32(-32768.0), r, np.float32(-32768.0))  # a NaN too
        r = np.where(r > np.float32(32767.0), np.float32(32767.0), r)
    return r.astype(np.int32)


def offsets(map_x, map_y, src_width, src_height, step, bpp):
    sx, sy = remap_index(map_x), remap_index(map_y)
    inside = (sx >= 0) & (sx < src_width) & (sy >= 0) & (sy < src_height)
    return np.where(inside, sy * np.int32(step) + sx * np.int32(bpp), np.int32(-1)).astype(np.int32)


def remap(src, map_x, map_y, src_width, src_height, encoding=0, step=0):
    """src: uint8, src_height rows of `step` bytes (0: src_width * bpp).  Returns uint8 [height, width * bpp]."""
    bpp = BPP[encoding]
    step = step or src_width * bpp
    flat = np.ascontiguousarray(src, np.uint8).reshape(-1)
    off = offsets(map_x, map_y, src_width, src_height, step, bpp)
    idx = np.where(off < 0, 0, off)[..., None] + np.arange(bpp)
    out = np.where((off >= 0)[..., None], flat[idx], np.uint8(0)).astype(np.uint8)
    return out.reshape(off.shape[0], off.shape[1] * bpp)


# ---- the argument checks (remap_plan.h); True: refused
def projector_check(cam):
    if cam is None:
        return True
    m = model_of(cam)
    if m == CAM_OCAM:
        return not np.isfinite(inv_poly_of(cam)).all()
    return kb.common_check(cam, 0)


def project_check(cam, n):
    return projector_check(cam) or n < 0 or n > MAX_POINTS


def build_check(cam, kind, width, height, M=None, have_x=True, have_y=True):
    if projector_check(cam) or kind not in (MAP_EQUIRECT, MAP_PERSPECTIVE):
        return True
    if kind == MAP_PERSPECTIVE and not np.isfinite(np.asarray(M, F64)).all():
        return True
    if not (MIN_SIDE <= width <= MAX_SIDE and MIN_SIDE <= height <= MAX_SIDE):
        return True
    return have_x != have_y


def apply_check(encoding, step, src_width, src_height):
    if encoding not in BPP or step < 0 or step > MAX_STEP:
        return True
    if not (MIN_SIDE <= src_width <= MAX_SIDE and MIN_SIDE <= src_height <= MAX_SIDE):
        return True
    return 0 < step < src_width * BPP[encoding]


def needs_rebuild(built, now):
    """The integer map was written for `built` = (src_width, src_height, step in bytes, bpp) or None; `now` likewise."""
    return built is None or tuple(built) != tuple(now)


# ---- the cameras, inputs and the cases of tests/golden/remap_cases.npz
# name -> (camera, (width, height)): the 13 of tests/test_camera_lift.py, the OCam pair with its inverse polynomial
CAMS = dict(PAL=(PAL, (synth.OCAM_W, synth.OCAM_H)), SKEW=(SKEW, (synth.OCAM_W, synth.OCAM_H)))
CAMS.update({n: (c, (cr.WIDTH, cr.HEIGHT)) for n, c in cr.CAMERAS.items()})
CAMS.update({n: (c, kb.SIZES[n]) for n, c in kb.CAMERAS.items()})
LIFT = {CAM_OCAM: tr.lift, CAM_PINHOLE: cr.lift, CAM_MEI: cr.lift, CAM_KANNALA_BRANDT: kb.lift}
NAN, INF, DENORMAL = float("nan"), float("inf"), 1e-310


def cam_vector(cam):
    """38 doubles, LfvioCamera's fields in order and the 20 of inv_poly; what a model does not read is 0."""
    g = lambda k: float(cam.get(k, 0.0))
    poly = [g("k2"), g("k3"), g("k4"), g("k5"), 0.0] if model_of(cam) == CAM_KANNALA_BRANDT else [float(v) for v in cam.get("poly", (0.0,) * 5)]
    kk = [0.0] * 4 if model_of(cam) == CAM_KANNALA_BRANDT else [g("k1"), g("k2"), g("p1"), g("p2")]
    inv = inv_poly_of(cam) if model_of(cam) == CAM_OCAM else np.zeros(INV_POLY_SIZE)
    return np.array([model_of(cam), g("cx"), g("cy"), g("c"), g("d"), g("e"), *poly, g("fx"), g("fy"), *kk, g("xi"), *inv], F64)


def cam_from_vector(v):
    m = int(v[0])
    if m == CAM_OCAM:
        return dict(model=m, cx=float(v[1]), cy=float(v[2]), c=float(v[3]), d=float(v[4]), e=float(v[5]), poly=tuple(float(x) for x in v[6:11]),
                    inv_poly=tuple(float(x) for x in v[18:38]))
    if m == CAM_KANNALA_BRANDT:
        return dict(model=m, cx=float(v[1]), cy=float(v[2]), fx=float(v[11]), fy=float(v[12]), k2=float(v[6]), k3=float(v[7]), k4=float(v[8]), k5=float(v[9]))
    cam = dict(model=m, cx=float(v[1]), cy=float(v[2]), fx=float(v[11]), fy=float(v[12]), k1=float(v[13]), k2=float(v[14]), p1=float(v[15]), p2=float(v[16]))
    if m == CAM_MEI:
        cam["xi"] = float(v[17])
    return cam


def special_rays():
    """The zero vector, the optical axis and its negative, X = Y = 0, Z = 0, and +-inf, NaN, a denormal in each component of a plain ray."""
    P = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 2.5], [-0.0, 0.0, -3.0], [1.0, 2.0, 0.0], [-1.0, 0.5, -0.0], [0.3, -0.2, 1.0],
         [1e-11, 0.0, 1.0], [0.0, -1e-12, -1.0], [1e-11, 1e-11, 0.0]]
    for k in range(3):
        for v in (INF, -INF, NAN, DENORMAL, -DENORMAL):
            r = [0.3, -0.2, 1.0]
            r[k] = v
            P.append(r)
    return np.array(P, F64)


def sphere_rays(name, n=4096):
    """Seeded rays over the whole sphere (z < 0 included), lengths from 0.1 to 30."""
    rng = np.random.default_rng([305, list(CAMS).index(name)])
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 30.0, (n, 1))


def image_rays(name, n=24, margin=12.0):
    """Rays of seeded pixels inside the camera's image: what a caller projects."""
    cam, (W, H) = CAMS[name]
    rng = np.random.default_rng([306, list(CAMS).index(name)])
    px = rng.uniform([margin, margin], [W - 1 - margin, H - 1 - margin], (n, 2)).astype(np.float32)
    return LIFT[model_of(cam)](cam, px) * rng.uniform(0.5, 20.0, (n, 1))


def fixture_rays(name):
    return np.concatenate([image_rays(name), sphere_rays(name, 16), special_rays()])


def noise_image(seed, width, height, encoding=0, step=0):
    """uint8 [height, step]: seeded noise, the padding bytes too (they must never show in an output)."""
    step = step or width * BPP[encoding]
    return np.random.default_rng([307, seed]).integers(0, 256, (height, step), dtype=np.uint8)


def look_down_M(width, height):
    """A perspective view of 90 degrees (f = width / 2) looking along -z: ray = R K^-1 (u, v, 1) with K = (f, f, width / 2, height / 2)
    and R = diag(1, -1, -1).  Divisions alone: the fixture's numbers do not depend on a libm."""
    f = width / 2.0
    return np.array([[1.0 / f, 0.0, -(width / 2.0) / f], [0.0, -1.0 / f, (height / 2.0) / f], [0.0, 0.0, -1.0]])


def K_inverse(cam):
    """M = K^-1 of a PINHOLE camera: with no distortion the PERSPECTIVE map is the identity."""
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    return np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])


# name: (camera, kind, width, height, M or None) — the small maps the fixture records; SRC_W x SRC_H is the source they gather from
SRC_W, SRC_H = 64, 48
MAPS = {
    "pal_equirect_33x17": ("PAL", MAP_EQUIRECT, 33, 17, None),
    "euroc_equirect_16x16": ("EUROC", MAP_EQUIRECT, 16, 16, None),
    "mv3dm_equirect_16x16": ("MV3DM", MAP_EQUIRECT, 16, 16, None),
    "tum_equirect_33x17": ("TUM", MAP_EQUIRECT, 33, 17, None),
    "pal_down_33x17": ("PAL", MAP_PERSPECTIVE, 33, 17, look_down_M(33, 17)),
    "euroc_nd_identity_37x16": ("EUROC_ND", MAP_PERSPECTIVE, 37, 16, K_inverse(cr.EUROC_ND)),
}
# what each recorded map gathers: (encoding, step)
GATHERS = ((0, 0), (2, 0), (2, 200), (4, 0), (6, 0))


def small(cam, s):
    """The camera of an image s times smaller (pixel quantities divided by s; OCam: centre and both polynomials in the pixel radius)."""
    if model_of(cam) != CAM_OCAM:
        return dict(cam, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=cam["cx"] / s, cy=cam["cy"] / s)
    return dict(cam, cx=cam["cx"] / s, cy=cam["cy"] / s, poly=tuple(c * s ** (i - 1) for i, c in enumerate(cam["poly"])),
                inv_poly=tuple(c / s for c in cam["inv_poly"]))


def map_case(name):
    """(camera, kind, width, height, M): the camera scaled so that its image is about SRC_W wide, and M's pixel part with it."""
    cam_name, kind, W, H, M = MAPS[name]
    cam, (cw, _) = CAMS[cam_name]
    s = cw / SRC_W
    if name == "euroc_nd_identity_37x16":
        return small(cam, s), kind, W, H, K_inverse(small(cam, s))
    return small(cam, s), kind, W, H, M
