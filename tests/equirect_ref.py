"""numpy specification of the lift of LFVIO_CAM_EQUIRECT (include/lfvio.h): the camera of the EXPANDED image that an
LFVIO_MAP_EQUIRECT map writes.  It is project_ref.equirect_rays' text (GetremapMat, pointcloud_image_fusion.cpp:93-101) with a tracked
point's float pixel in place of the integer (i, j), one rounding per operation, grouped as written:

  lon = ((double)px / fx - 0.5) * (2.0 * pi),  lat = -(((double)py / fy - 0.5) * pi),  P = (cos lat sin lon, cos lat cos lon, sin lat)

with fx, fy the image's width and height and sine and cosine by kb_ref.sincos.  lf-vio_amd/csrc/camera_models.h (cam_lift_equirect) is
the same text in C++ for the host and the device; tests/test_equirect_lift.py holds it to this file bit for bit, this file to the map's
own rays at integer pixels and to a 50-digit evaluation of the definition.  Everything behind the lift is track_ref's."""
import numpy as np

import kb_ref as kb
import track_ref as tr
import twoview_ref as tv

F64 = np.float64
CAM_EQUIRECT = 6
MIN_SIDE, MAX_SIDE = 16, 8192
PI, TWO_PI = F64(np.pi), F64(2.0) * F64(np.pi)


def camera(width, height):
    return dict(model=CAM_EQUIRECT, fx=float(width), fy=float(height))


def angles(cam, px):
    """(lon, lat) float64 of pixels px [..., 2] float32."""
    px = np.asarray(px, np.float32)
    with np.errstate(all="ignore"):
        lon = (px[..., 0].astype(F64) / F64(cam["fx"]) - F64(0.5)) * TWO_PI
        lat = -((px[..., 1].astype(F64) / F64(cam["fy"]) - F64(0.5)) * PI)
    return lon, lat


def lift(cam, px):
    """px [..., 2] float32 -> P [..., 3] float64."""
    lon, lat = angles(cam, px)
    with np.errstate(all="ignore"):
        slon, clon = kb.sincos(lon)
        slat, clat = kb.sincos(lat)
        return np.stack([clat * slon, clat * clon, slat], axis=-1)


norm = tr.norm


def bearings(cam, px):
    P = lift(cam, px)
    with np.errstate(all="ignore"):
        return P / norm(P)[..., None]


def undistorted(cam, px):
    """(un_pts [N, 2], un_pts_3d [N, 3]) float32: the quotients in double, rounded once."""
    P = lift(cam, np.asarray(px, np.float32).reshape(-1, 2))
    with np.errstate(all="ignore"):
        return np.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]], axis=-1).astype(np.float32), (P / norm(P)[:, None]).astype(np.float32)


# ---- the argument check (track_camera_check, camera_models.h); True: refused
def camera_check(cam):
    if cam is None:
        return True
    for k in ("fx", "fy"):
        x = float(cam[k])
        if not (MIN_SIDE <= x <= MAX_SIDE) or x != np.floor(x):  # (a NaN fails the comparison)
            return True
    return False


def common_check(cam, N):
    if cam is None or cam.get("model", 0) != CAM_EQUIRECT:
        return kb.common_check(cam, N)
    return camera_check(cam) or N < 0 or N > tr.MAX_POINTS


# ---- rejectWithF and undistortedPoints: track_ref's flow over this file's lift
def reject(cam, cur_pts, forw_pts, samples):
    """track_ref.reject's dict, over this file's bearings."""
    cur, forw = np.asarray(cur_pts, np.float32).reshape(-1, 2), np.asarray(forw_pts, np.float32).reshape(-1, 2)
    N = len(cur)
    if N < tr.MIN_MATCHES:
        return dict(status=2, mask=np.ones(N, np.uint8), best_sample=-1, num_inliers=0, best_score=0.0)
    bl, br = bearings(cam, cur), bearings(cam, forw)
    r = tv.two_view(bl, br, samples)
    out = dict(status=int(r["status"]), best_sample=int(r["best_sample"]), num_inliers=int(r["num_inliers"]), best_score=float(r["best_score"]),
               bearing_cur=bl, bearing_forw=br)
    if r["status"] == 0:
        out.update(mask=np.asarray(r["mask"], np.uint8), E=r["E"])
    else:
        out.update(mask=np.ones(N, np.uint8))
    return out


class Undistort(tr.Undistort):
    """track_ref.Undistort (the insert-once map and the time) with this file's lift."""

    def __call__(self, cam, pts, ids, time):
        pts, ids = np.asarray(pts, np.float32).reshape(-1, 2), np.asarray(ids, np.int32).reshape(-1)
        N = len(pts)
        un, un3 = undistorted(cam, pts)
        with np.errstate(all="ignore"):
            vel, matched = np.zeros((N, 3), np.float32), np.full(N, -1, np.int32)
            first = {}
            for j, k in enumerate(self.ids.tolist()):
                first.setdefault(k, j)
            dt = np.float64(time) - np.float64(self.time)
            for i in range(N):
                j = first.get(int(ids[i]), -1) if ids[i] != -1 else -1
                if j >= 0:
                    matched[i] = j
                    vel[i] = ((un3[i] - self.p3d[j]).astype(np.float64) / dt).astype(np.float32)  # the difference in float
        self.ids, self.p3d, self.time = ids.copy(), un3.copy(), float(time)
        return dict(un_pts=un, un_pts_3d=un3, velocity_3d=vel, matched=matched)


# ---- inputs
def project(cam, P):
    """The pixel of rays P [N, 3] (only test inputs are made with it): the inverse of the lift, by libm."""
    P = np.asarray(P, F64)
    lon = np.arctan2(P[:, 0], P[:, 1])
    lat = np.arctan2(P[:, 2], np.hypot(P[:, 0], P[:, 1]))
    return np.stack([(lon / (2.0 * np.pi) + 0.5) * cam["fx"], (0.5 - lat / np.pi) * cam["fy"]], axis=-1)


def make_matches(seed, cam, N, noise_px=0.5, outliers=0.2):
    """(cur, forw) float32 [N, 2]: N points seen from two poses a small rotation and translation apart, away from the poles and the
    seam, pixel noise on both, and a share of `outliers` whose second pixel is drawn anew."""
    rng = np.random.default_rng([311, seed])
    lon, lat = rng.uniform(-2.6, 2.6, N), rng.uniform(-1.0, 1.0, N)
    X = np.stack([np.cos(lat) * np.sin(lon), np.cos(lat) * np.cos(lon), np.sin(lat)], axis=-1) * rng.uniform(2.0, 12.0, (N, 1))
    w = np.array([0.01, -0.02, 0.015])
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    R = np.eye(3) + K + 0.5 * K @ K
    X2 = X @ R.T + np.array([0.12, -0.05, 0.08])
    cur = project(cam, X) + rng.normal(0.0, noise_px, (N, 2))
    forw = project(cam, X2) + rng.normal(0.0, noise_px, (N, 2))
    bad = rng.random(N) < outliers
    forw[bad] = rng.uniform([2.0, 2.0], [cam["fx"] - 2.0, cam["fy"] - 2.0], (int(bad.sum()), 2))
    return cur.astype(np.float32), forw.astype(np.float32)
