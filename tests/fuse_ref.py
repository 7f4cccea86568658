"""numpy specification of lfvio_cloud_fuse (include/lfvio.h): a lidar scan's points into the camera frame, through the
range gate, onto their pixels of the equirectangular image (the inverse of project_ref.equirect_rays) or of a camera's own image
(project_ref.project), the range image, the colours under the points and the painted image; one rounding per operation.
lf-vio_amd/csrc/fuse_plan.h is the same text in C++ for the host and the device; it is held to this file bit for bit
(tests/test_fuse_plan.py, tests/test_fuse_gpu.py), and this file to a 50-digit evaluation of the reference's definition
(pointcloud_image_fusion_node.cpp:92-115: normalise, atan2(x, y), asin(z), the two index lines; tests/test_fuse_ref.py).

  fields          the float32 fields x, y, z of a sensor_msgs/PointCloud2's data bytes, either byte order, any alignment
  pack_cloud      the other way, for the tests: noise in every byte that is not a field
  transform       P.k = ((R[3k] x + R[3k + 1] y) + R[3k + 2] z) + T[k]
  lon             the angle of atan2(X, Y) on project_ref.atan, as project_ref.kb_theta builds its angle
  equirect_frac   (fx, fy), the fractional pixel
  points          (index, range, why) of every point: FuseHit of fuse_plan.h
  range_image     the smallest range per pixel, +inf where there is none
  fuse            everything lfvio_cloud_fuse returns
  check           the argument check of fuse_plan.h; True: refused"""
import numpy as np

import project_ref as pr

F64, F32 = np.float64, np.float32
FUSE_EQUIRECT, FUSE_CAMERA = 0, 1
IMAGE_NONE, IMAGE_GIVEN, IMAGE_REMAP = 0, 1, 2
KEPT, GATE, PROJECTION = 0, 1, 2
MAX_POINTS, MIN_STEP, MAX_STEP = 1 << 20, 12, 1024
PI = F64(3.14159265358979323846)


# ---- the cloud's bytes
def fields(data, n, point_step, off_x, off_y, off_z, big_endian=0):
    """-> (x, y, z) float32 [n] from n * point_step bytes."""
    b = np.frombuffer(bytes(data), np.uint8, count=n * point_step).reshape(n, point_step)
    dt = ">f4" if big_endian else "<f4"
    return tuple(np.ascontiguousarray(b[:, o:o + 4]).view(dt).reshape(n).astype(F32) for o in (off_x, off_y, off_z))


def pack_cloud(xyz, point_step=12, offs=(0, 4, 8), big_endian=0, seed=0):
    """uint8 [n * point_step]: the three float32 fields at `offs`, seeded noise in every other byte (it must never show)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    b = np.random.default_rng([401, seed]).integers(0, 256, (len(xyz), point_step), dtype=np.uint8)
    for k, o in enumerate(offs):
        b[:, o:o + 4] = np.ascontiguousarray(xyz[:, k]).astype(">f4" if big_endian else "<f4").view(np.uint8).reshape(-1, 4)
    return b.reshape(-1)


# ---- per point
def transform(R, T, x, y, z):
    R, T = np.asarray(R, F64).reshape(9), np.asarray(T, F64).reshape(3)
    x, y, z = (np.asarray(v, F32).astype(F64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        return tuple(((R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] * z) + T[k] for k in range(3))


def lon(X, Y):
    """The angle of atan2(X, Y): 0 along +Y, positive towards +X.  Y > 0: atan(X / Y); Y < 0: pi + atan, or atan - pi for X < 0, pi in
    its two parts; Y == 0: +-pi / 2 by the sign of X."""
    with np.errstate(all="ignore"):
        a = pr.atan(X / Y)
        behind = np.where(X >= 0.0, pr.PI_HI + (a + pr.PI_LO), (a - pr.PI_LO) - pr.PI_HI)
        side = np.where(X > 0.0, pr.PIO2, np.where(X < 0.0, -pr.PIO2, a))
        return np.where(Y > 0.0, a, np.where(Y < 0.0, behind, side))


def equirect_frac(width, height, X, Y, Z):
    """(fx, fy) float64: fx = width (0.5 + lon / (2 pi)), fy = height (0.5 - lat / pi), lat = atan(Z / nxy)."""
    with np.errstate(all="ignore"):
        nxy = np.sqrt(X * X + Y * Y)
        lat = pr.atan(Z / nxy)
        return F64(width) * (F64(0.5) + lon(X, Y) / (F64(2.0) * PI)), F64(height) * (F64(0.5) - lat / PI)


def view(kind=FUSE_EQUIRECT, width=960, height=480, R=np.eye(3), T=(0.0, 0.0, 0.0), min_range=0.0, max_range=np.inf, cam=None):
    return dict(kind=kind, width=width, height=height, R=np.asarray(R, F64).reshape(9), T=np.asarray(T, F64).reshape(3), min_range=float(min_range),
                max_range=float(max_range), cam=cam)


def points(v, x, y, z):
    """-> (index int32 [n], range float32 [n], why int32 [n])."""
    W, H = v["width"], v["height"]
    X, Y, Z = transform(v["R"], v["T"], x, y, z)
    with np.errstate(all="ignore"):
        r = np.sqrt((X * X + Y * Y) + Z * Z)
        rf = r.astype(F32)
        gate = (r > 0.0) & (r >= F64(v["min_range"])) & (r <= F64(v["max_range"])) & (r < np.inf)
        if v["kind"] == FUSE_EQUIRECT:
            nxy = np.sqrt(X * X + Y * Y)
            ok = gate & (nxy != 0.0)
            fx, fy = equirect_frac(W, H, X, Y, Z)
            col = np.where(ok, fx, 0.0).astype(np.int32)  # truncation; both >= 0
            row = np.where(ok, fy, 0.0).astype(np.int32)
            col = np.where(col == W, 0, col)
            row = np.where(row == H, H - 1, row)
        else:
            cam = v["cam"]
            uv = pr.project(cam, np.stack([X, Y, Z], axis=-1))
            col, row = pr.remap_index(uv[..., 0].astype(F32)), pr.remap_index(uv[..., 1].astype(F32))
            m = pr.model_of(cam)
            front = Z > 0.0 if m == pr.CAM_PINHOLE else (Z + F64(cam["xi"]) * r > 0.0 if m == pr.CAM_MEI else np.ones(r.shape, bool))
            ok = gate & front
        ok = ok & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    index = np.where(ok, row * np.int32(W) + col, np.int32(-1)).astype(np.int32)
    why = np.where(ok, KEPT, np.where(gate, PROJECTION, GATE)).astype(np.int32)
    return index, rf, why


def range_image(index, rf, width, height):
    out = np.full(width * height, np.inf, F32)
    kept = index >= 0
    np.minimum.at(out, index[kept], rf[kept])
    return out.reshape(height, width)


def counts(why):
    return np.array([(why == k).sum() for k in (KEPT, GATE, PROJECTION)], np.int32)


def fuse(v, x, y, z, image=None, bpp=0, paint=None):
    """image: uint8 [height, width * bpp], rows contiguous (a remapped source: project_ref.remap's output), or None.  paint: None, or
    the bytes written at every marked pixel (the first bpp).  -> dict(index, range, counts, colour, image_out); the last two None
    without an image."""
    index, rf, why = points(v, x, y, z)
    out = dict(index=index, range=range_image(index, rf, v["width"], v["height"]), counts=counts(why), colour=None, image_out=None)
    if image is None:
        return out
    px = np.ascontiguousarray(image, np.uint8).reshape(v["width"] * v["height"], bpp)
    kept = index >= 0
    out["colour"] = np.where(kept[:, None], px[np.where(kept, index, 0)], np.uint8(0)).astype(np.uint8)
    painted = px.copy()
    if paint is not None:
        painted[index[kept]] = np.asarray(paint, np.uint8)[:bpp]
    out["image_out"] = painted.reshape(v["height"], v["width"] * bpp)
    return out


# ---- the argument check (fuse_plan.h); True: refused
def check(n=1, point_step=12, offs=(0, 4, 8), big_endian=0, R=np.eye(3), T=(0.0, 0.0, 0.0), min_range=0.0, max_range=np.inf, kind=FUSE_EQUIRECT,
          width=33, height=17, cam=None, image_mode=IMAGE_NONE, encoding=0, step=0, src_width=64, src_height=48, want_colour=False, want_image=False):
    if n < 0 or n > MAX_POINTS or point_step < MIN_STEP or point_step > MAX_STEP:
        return True
    if any(o < 0 or o > point_step - 4 for o in offs):
        return True
    if any(abs(offs[a] - offs[b]) < 4 for a, b in ((0, 1), (0, 2), (1, 2))):
        return True
    if big_endian not in (0, 1) or not np.isfinite(np.asarray(R, F64)).all() or not np.isfinite(np.asarray(T, F64)).all():
        return True
    if not np.isfinite(min_range) or min_range < 0.0 or not max_range >= min_range:
        return True
    if kind not in (FUSE_EQUIRECT, FUSE_CAMERA) or not (pr.MIN_SIDE <= width <= pr.MAX_SIDE and pr.MIN_SIDE <= height <= pr.MAX_SIDE):
        return True
    if kind == FUSE_CAMERA and pr.projector_check(cam):
        return True
    if image_mode not in (IMAGE_NONE, IMAGE_GIVEN, IMAGE_REMAP):
        return True
    if image_mode == IMAGE_NONE:
        return want_colour or want_image
    return pr.apply_check(encoding, step, *((width, height) if image_mode == IMAGE_GIVEN else (src_width, src_height)))


# ---- the inputs of the tests and of tests/golden/fuse_cases.npz
def node_R():
    """camera_R_lidar as the node writes it (pointcloud_image_fusion_node.cpp:96-98), theta = pi / 2; with T = (0, 0, -0.12)."""
    th = np.pi / 2
    return np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), -np.cos(th), 0.0], [0.0, 0.0, 1.0]])


NODE_T = (0.0, 0.0, -0.12)


def random_R(seed=0):
    q, _ = np.linalg.qr(np.random.default_rng([402, seed]).normal(size=(3, 3)))
    return q


def poses():
    return (("identity", np.eye(3), (0.0, 0.0, 0.0)), ("node", node_R(), NODE_T), ("random", random_R(), (0.3, -0.2, 0.1)))


def sphere_cloud(n=20000, seed=0, lo=0.3, hi=120.0):
    """Seeded points over the whole sphere at ranges lo .. hi m, float32 [n, 3]."""
    rng = np.random.default_rng([403, seed])
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))).astype(F32)


def camera_cloud(name, n, seed=0):
    """Half the points on rays of pixels inside the camera's image, half over the whole sphere (behind the camera too)."""
    a = pr.image_rays(name, n - n // 2).astype(F32)
    return np.concatenate([a, sphere_cloud(n // 2, seed=seed + 50, lo=0.5, hi=30.0)])[np.random.default_rng([404, seed]).permutation(n)]


def special_cloud():
    """Zeros, NaN and +-inf in each coordinate, huge and tiny values, the seam, the axes and the poles."""
    nan, inf = np.nan, np.inf
    P = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0],
         [1e-30, -1.0, 0.0], [-1e-30, -1.0, 0.0], [1e-3, -1.0, 0.2], [-1e-3, -1.0, -0.2], [1e-30, 0.0, 1.0], [0.0, 1e-30, -1.0], [3e38, 1.0, 1.0],
         [1e-40, 1e-40, 1e-40], [1e-25, 1e-25, 1.0], [1e-25, 0.0, -1.0], [2.0, 3.0, -1.0], [0.5, 0.5, 0.5]]
    for k in range(3):
        for v in (nan, inf, -inf):
            p = [1.0, 2.0, 0.5]
            p[k] = v
            P.append(p)
    return np.array(P, F32)
