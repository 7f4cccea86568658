"""numpy restatement of the tracker calls for the PINHOLE and MEI camera models (include/lfvio.h): the specification of
PinholeCamera::liftProjective (camera_model/src/camera_models/PinholeCamera.cc:450-510) and CataCamera::liftProjective
(CataCamera.cc:556-626) as lfvio_track_reject / lfvio_track_undistort and the frame calls use them.  Everything behind the lift is
tests/track_ref.py's and twoview_ref's, imported; an OCam camera is delegated to track_ref throughout.

  host_constants   what track_plan.h's track_cam forms once, on the host: inv11, inv13, inv22, inv23, no_distortion
  lift, bearings   the lift in double, one rounding per operation, grouped as the reference's source reads left to right, and P / n
                   with track_ref.norm.  Nobody has compared this with the reference's Eigen build (it does not build here).
  reject           track_ref.reject over this file's bearings
  Undistort        track_ref.Undistort over this file's lift
  common_check, reject_check, undistort_check   the argument checks of track_plan.h; True: refused
  project          spaceToPlane (inputs only: its bits are nobody's specification)
  make_matches, make_samples, undistort_sequence, CASES, make_case   inputs and the fixture cases of tests/golden/camera_cases.npz

A camera is a dict: model, cx, cy, fx, fy, k1, k2, p1, p2 and, for MEI, xi (MEI's u0, v0, gamma1, gamma2 under cx, cy, fx, fy)."""
import numpy as np

import track_ref as tr
import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio import synth

CAM_OCAM, CAM_PINHOLE, CAM_MEI = 0, 2, 3
WIDTH, HEIGHT = 752, 480

# the reference's settings (config/euroc, config/3dm), as numbers
EUROC = dict(model=CAM_PINHOLE, fx=461.6, fy=460.3, cx=363.0, cy=248.1, k1=-0.2917, k2=0.08228, p1=5.333e-05, p2=-1.578e-04)
MV3DM = dict(model=CAM_MEI, fx=1115.0, fy=1114.0, cx=367.2, cy=238.5, xi=2.057, k1=0.07145, k2=0.5059, p1=4.727e-05, p2=-5.492e-04)
EUROC_ND = dict(EUROC, k1=0.0, k2=0.0, p1=0.0, p2=0.0)  # the no_distortion branch
MV3DM_ND = dict(MV3DM, k1=0.0, k2=0.0, p1=0.0, p2=0.0)
MEI_XI1 = dict(MV3DM, xi=1.0)  # the xi == 1.0 branch
CAMERAS = dict(EUROC=EUROC, MV3DM=MV3DM, EUROC_ND=EUROC_ND, MV3DM_ND=MV3DM_ND, MEI_XI1=MEI_XI1)


def model_of(cam):
    return cam.get("model", CAM_OCAM)


def scaled(cam, s):
    """The camera of an image s times smaller: the pixel quantities divided by s."""
    return dict(cam, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=cam["cx"] / s, cy=cam["cy"] / s)


# ---- the lift
def host_constants(cam):
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    nd = all(np.float64(cam[k]) == 0.0 for k in ("k1", "k2", "p1", "p2"))
    return dict(inv11=np.float64(1.0) / fx, inv13=-cx / fx, inv22=np.float64(1.0) / fy, inv23=-cy / fy, no_distortion=bool(nd))


def _dist(cam, x, y):
    k1, k2, p1, p2 = (np.float64(cam[k]) for k in ("k1", "k2", "p1", "p2"))
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + (k2 * rho2) * rho2
    dx = (x * rad + (np.float64(2.0) * p1) * mxy) + p2 * (rho2 + np.float64(2.0) * mx2)
    dy = (y * rad + (np.float64(2.0) * p2) * mxy) + p1 * (rho2 + np.float64(2.0) * my2)
    return dx, dy


def lift(cam, px):
    """px [..., 2] float32 -> P [..., 3] float64."""
    if model_of(cam) == CAM_OCAM:
        return tr.lift(cam, px)
    px = np.asarray(px, np.float32)
    h = host_constants(cam)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        mx_d = h["inv11"] * px[..., 0].astype(np.float64) + h["inv13"]
        my_d = h["inv22"] * px[..., 1].astype(np.float64) + h["inv23"]
        mx_u, my_u = mx_d, my_d
        if not h["no_distortion"]:
            for _ in range(8):
                dx, dy = _dist(cam, mx_u, my_u)
                mx_u, my_u = mx_d - dx, my_d - dy
        if model_of(cam) == CAM_PINHOLE:
            z = np.ones_like(mx_u)
        else:
            xi = np.float64(cam["xi"])
            if xi == 1.0:
                z = ((one - mx_u * mx_u) - my_u * my_u) / np.float64(2.0)
            else:
                rho2 = mx_u * mx_u + my_u * my_u
                z = one - (xi * (rho2 + one)) / (xi + np.sqrt(one + (one - xi * xi) * rho2))
    return np.stack([mx_u, my_u, z], axis=-1)


norm = tr.norm


def bearings(cam, px):
    P = lift(cam, px)
    with np.errstate(all="ignore"):
        return P / norm(P)[..., None]


def project(cam, P):
    """spaceToPlane of rays P [N, 3] (only the test inputs are made with it)."""
    if model_of(cam) == CAM_OCAM:
        return tr.project(cam, P)
    return synth.camera_space_to_plane(cam, P)


# ---- the argument checks (track_plan.h); True: refused
def common_check(cam, N):
    if cam is None:
        return True
    m = model_of(cam)
    if m == CAM_OCAM:
        return tr.common_check(cam, N)
    if m not in (CAM_PINHOLE, CAM_MEI):
        return True
    if not all(np.isfinite(cam[k]) for k in ("cx", "cy", "fx", "fy", "k1", "k2", "p1", "p2")):
        return True
    if cam["fx"] == 0.0 or cam["fy"] == 0.0:
        return True
    if m == CAM_MEI and not np.isfinite(cam["xi"]):
        return True
    return N < 0 or N > tr.MAX_POINTS


def reject_check(cam, N, have_cur, have_forw, S, samples):
    if common_check(cam, N):
        return True
    return tr.reject_check(tr.PAL, N, have_cur, have_forw, S, samples)  # (the rest does not look at the camera)


def undistort_check(cam, N, have_pts, have_ids, time):
    if common_check(cam, N):
        return True
    return tr.undistort_check(tr.PAL, N, have_pts, have_ids, time)


# ---- rejectWithF
def reject(cam, cur_pts, forw_pts, samples):
    """track_ref.reject's dict, over this file's bearings."""
    if model_of(cam) == CAM_OCAM:
        return tr.reject(cam, cur_pts, forw_pts, samples)
    cur, forw = np.asarray(cur_pts, np.float32).reshape(-1, 2), np.asarray(forw_pts, np.float32).reshape(-1, 2)
    N = len(cur)
    if N < tr.MIN_MATCHES:
        return dict(status=2, mask=np.ones(N, np.uint8), best_sample=-1, num_inliers=0, best_score=0.0)
    bl, br = bearings(cam, cur), bearings(cam, forw)
    r = tv.two_view(bl, br, samples)
    out = dict(status=int(r["status"]), best_sample=int(r["best_sample"]), num_inliers=int(r["num_inliers"]), best_score=float(r["best_score"]),
               bearing_cur=bl, bearing_forw=br, c1_gap=r.get("c1_gap", np.inf), c2_margin=r.get("c2_margin", np.inf))
    if r["status"] == 0:
        out.update(mask=np.asarray(r["mask"], np.uint8), E=r["E"])
    else:
        out.update(mask=np.ones(N, np.uint8))
    return out


conditions = tr.conditions


# ---- undistortedPoints
class Undistort(tr.Undistort):
    """track_ref.Undistort (the insert-once map and the time) with this file's lift."""

    def __call__(self, cam, pts, ids, time):
        if model_of(cam) == CAM_OCAM:
            return super().__call__(cam, pts, ids, time)
        pts, ids = np.asarray(pts, np.float32).reshape(-1, 2), np.asarray(ids, np.int32).reshape(-1)
        N = len(pts)
        P = lift(cam, pts)
        with np.errstate(all="ignore"):
            un = np.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]], axis=-1).astype(np.float32)
            un3 = (P / norm(P)[:, None]).astype(np.float32)
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
MARGIN = 12.0  # pixels between a drawn pixel and the image's edge: 1 px of noise stays inside


def _inside(px):
    return (px[:, 0] >= MARGIN) & (px[:, 0] <= WIDTH - 1 - MARGIN) & (px[:, 1] >= MARGIN) & (px[:, 1] <= HEIGHT - 1 - MARGIN)


def make_matches(seed, cam, N, noise_px=1.0, outliers=0.2):
    """A rigid two-view motion of points in front of the camera, seen through it: (cur_pts, forw_pts) float32 [N, 2] inside
    WIDTH x HEIGHT, with noise_px of Gaussian noise on both pixels and a share of gross outliers (forw pixels drawn anew)."""
    rng = np.random.default_rng([seed, 4099])
    R = gen.rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0.5, 6.0)))
    d = rng.normal(size=3)
    t = rng.uniform(0.05, 0.5) * d / np.linalg.norm(d)
    cur, forw = np.zeros((0, 2)), np.zeros((0, 2))
    while len(cur) < N:
        px = rng.uniform([MARGIN, MARGIN], [WIDTH - 1 - MARGIN, HEIGHT - 1 - MARGIN], (2 * N, 2))
        ray = synth.camera_lift(cam, px)
        X = ray / np.linalg.norm(ray, axis=1, keepdims=True) * rng.uniform(2.0, 12.0, (2 * N, 1))
        Xr = X @ R.T + t
        q = project(cam, Xr)
        ok = np.isfinite(q).all(axis=1) & _inside(np.nan_to_num(q)) & (Xr[:, 2] > 0.5)
        cur, forw = np.vstack([cur, project(cam, X)[ok]]), np.vstack([forw, q[ok]])
    cur = cur[:N] + rng.normal(0.0, noise_px, (N, 2))
    forw = forw[:N] + rng.normal(0.0, noise_px, (N, 2))
    bad = rng.random(N) < outliers
    forw[bad] = rng.uniform([MARGIN, MARGIN], [WIDTH - 1 - MARGIN, HEIGHT - 1 - MARGIN], (int(bad.sum()), 2))
    hi = np.array([WIDTH - 1.0, HEIGHT - 1.0])
    return np.clip(cur, 0.0, hi).astype(np.float32), np.clip(forw, 0.0, hi).astype(np.float32)


make_samples = tr.make_samples


def cone(rng, n, cam):
    """Rays in front of the camera whose pixels are inside the image: the lift of uniform pixels."""
    px = rng.uniform([3 * MARGIN, 3 * MARGIN], [WIDTH - 1 - 3 * MARGIN, HEIGHT - 1 - 3 * MARGIN], (n, 2))
    ray = synth.camera_lift(cam, px)
    return ray / np.linalg.norm(ray, axis=1, keepdims=True)


def undistort_sequence(seed, cam, calls=4, N=40):
    """track_ref.undistort_sequence for a camera of this file: ids that stay, vanish, arrive as -1 and are numbered afterwards, a
    duplicate."""
    rng = np.random.default_rng([seed, 17])
    ids = np.arange(N, dtype=np.int32)
    nxt, seq = N, []
    P = cone(rng, N, cam)
    for k in range(calls):
        P = P + rng.normal(0.0, 0.004, P.shape)
        pts = (project(cam, P) + rng.normal(0.0, 0.3, (len(P), 2))).astype(np.float32)
        call_ids = ids.copy()
        if k == 2:
            call_ids[5] = call_ids[3]  # a duplicate
        seq.append((pts, call_ids.copy(), 0.05 * k + 1.0))
        for i in range(len(ids)):  # the caller numbers the -1s, drops a few, detects new corners
            if ids[i] == -1:
                ids[i], nxt = nxt, nxt + 1
        keep = rng.random(len(ids)) > 0.15
        new = int((~keep).sum())
        P = np.concatenate([P[keep], cone(rng, new, cam)])
        ids = np.concatenate([ids[keep], np.full(new, -1, np.int32)])
    return seq


KEYS = ("model", "cx", "cy", "fx", "fy", "k1", "k2", "p1", "p2", "xi")


def cam_vector(cam):
    return np.array([cam.get(k, 0.0) for k in KEYS], np.float64)


def cam_from_vector(v):
    cam = dict(zip(KEYS, (float(x) for x in v)))
    cam["model"] = int(v[0])
    return cam


# name: (camera, seed, N, S)
CASES = {
    "euroc_60": ("EUROC", 11, 60, 100),
    "mv3dm_97": ("MV3DM", 12, 97, 100),
    "euroc_nd_80": ("EUROC_ND", 13, 80, 100),
    "mv3dm_nd_45": ("MV3DM_ND", 14, 45, 100),
    "mei_xi1_70": ("MEI_XI1", 15, 70, 100),
    "euroc_8": ("EUROC", 16, 8, 4),
    "mv3dm_7": ("MV3DM", 17, 7, 4),
}


def small(N):
    """make_matches' noise for N matches: with fewer than 30 every match is needed, so little noise and no outlier."""
    return dict(noise_px=0.05, outliers=0.0) if N < 30 else {}


def make_case(name):
    cam_name, seed, N, S = CASES[name]
    cam = CAMERAS[cam_name]
    cur, forw = make_matches(seed, cam, N, **small(N))
    return cam, cur, forw, make_samples(seed + 500, max(N, 8), S) % max(N, 1)
