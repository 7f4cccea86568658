"""numpy specification of the KANNALA_BRANDT camera model's lift (include/lfvio.h) as lfvio_track_reject /
lfvio_track_undistort and the frame calls use it: EquidistantCamera::liftProjective (camera_model/src/camera_models/
EquidistantCamera.cc:428-442) over backprojectSymmetric (:716-818), restated in operations IEEE 754 defines (+ - * / sqrt floor and
comparisons), one rounding per operation.  lf-vio_amd/csrc/camera_kb.h is the same text in C++, for the host and the device; both are
held to this file bit for bit, and this file to a 50-digit evaluation of the reference's definition (tests/test_kb_ref.py).

  host_constants   what track_plan.h forms once per camera: inv11, inv13, inv22, inv23, theta_lim, r_lim
  root             the smallest non-negative real root of theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 = r on the monotone
                   range [0, theta_lim] by NEWTON_STEPS clamped Newton steps; theta = r beyond r_lim and for a NaN (:809-812)
  sincos           sin and cos by a three-part Cody-Waite reduction by pi / 2 and the fdlibm kernels
  lift, bearings   (sin theta x / r, sin theta y / r, cos theta), and P / n with track_ref.norm
  reject, Undistort, conditions   track_ref's, over this file's lift
  common_check, reject_check, undistort_check   the argument checks of track_plan.h; True: refused
  project          spaceToPlane (:450-470; inputs only: its bits are nobody's specification)
  CAMERAS, SIZES, CASES, make_case, make_matches, undistort_sequence   the cameras, inputs and the cases of tests/golden/kb_cases.npz

Deviations from the reference's text, stated: x / r, y / r in place of cos(atan2(y, x)), sin(atan2(y, x)); Newton's method in place of
the eigenvalues of the companion matrix; a root behind a dip of the polynomial inside [0, pi] is not looked for (none of the shipped
calibrations has one); the pi / 4096 grid can miss a dip of f' narrower than a grid step.

A camera is a dict: model, cx, cy, fx, fy (the YAML's u0, v0, mu, mv) and k2, k3, k4, k5."""
import numpy as np

import camera_ref as cr
import track_ref as tr
import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio import synth

CAM_KANNALA_BRANDT = 5
NEWTON_STEPS = 13  # the most the sweep of tests/test_kb_ref.py needs to reach the residual bar, plus two
GRID = 4096
F64 = np.float64

# the reference's settings (config/tum, config/cla, config/realsense/realsense_fisheye_config.yaml), as numbers
TUM = dict(model=5, k2=0.0034823894022493434, k3=0.0007150348452162257, k4=-0.0020532361418706202, k5=0.00020293673591811182,
           fx=190.97847715128717, fy=190.9733070521226, cx=254.93170605935475, cy=256.8974428996504)
CLA = dict(model=5, k2=-0.005740195474458931, k3=0.02878252863739417, k4=-0.04010621197185408, k5=0.02008469575876223,
           fx=472.2863830700696, fy=470.83759684346785, cx=368.8316828103749, cy=232.23688706965652)
RSFISH = dict(model=5, k2=1.7280355035195181e-02, k3=-2.5505200860040985e-02, k4=2.2621441637715487e-02, k5=-7.3355871719731113e-03,
              fx=2.7723712054408202e+02, fy=2.7699784668734617e+02, cx=3.3625356873985868e+02, cy=2.3603924727453901e+02)
KB_K5_0 = dict(CLA, k5=0.0)
KB_K45_0 = dict(CLA, k4=0.0, k5=0.0)
KB_IDEAL = dict(CLA, k2=0.0, k3=0.0, k4=0.0, k5=0.0)
CAMERAS = dict(TUM=TUM, CLA=CLA, RSFISH=RSFISH, KB_K5_0=KB_K5_0, KB_K45_0=KB_K45_0, KB_IDEAL=KB_IDEAL)
SIZES = dict(TUM=(512, 512), CLA=(752, 480), RSFISH=(640, 480), KB_K5_0=(752, 480), KB_K45_0=(752, 480), KB_IDEAL=(752, 480))


def scaled(cam, s):
    """The camera of an image s times smaller: the pixel quantities divided by s."""
    return dict(cam, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=cam["cx"] / s, cy=cam["cy"] / s)


def ks(cam):
    return tuple(F64(cam[k]) for k in ("k2", "k3", "k4", "k5"))


# ---- the polynomial, as Horner forms
def f_poly(k, th):
    """theta (1 + t (k2 + t (k3 + t (k4 + t k5)))), t = theta theta."""
    k2, k3, k4, k5 = k
    t = th * th
    return th * (F64(1.0) + t * (k2 + t * (k3 + t * (k4 + t * k5))))


def fp_poly(k, th):
    """1 + t (3 k2 + t (5 k3 + t (7 k4 + t 9 k5))): the four products of the coefficients are rounded once each."""
    k2, k3, k4, k5 = k
    t = th * th
    return F64(1.0) + t * (F64(3.0) * k2 + t * (F64(5.0) * k3 + t * (F64(7.0) * k4 + t * (F64(9.0) * k5))))


def host_constants(cam):
    fx, fy, cx, cy = (F64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k = ks(cam)
    step = F64(np.pi) / F64(GRID)
    lim = F64(0.0)  # f'(0) = 1
    with np.errstate(all="ignore"):
        for j in range(1, GRID + 1):
            th = F64(j) * step
            if not fp_poly(k, th) > 0.0:
                break
            lim = th
        r_lim = f_poly(k, lim)
    return dict(inv11=F64(1.0) / fx, inv13=-cx / fx, inv22=F64(1.0) / fy, inv23=-cy / fy, theta_lim=lim, r_lim=r_lim)


def newton(k, lim, r, steps):
    """`steps` clamped Newton steps from min(r, theta_lim), every select written so that a NaN falls through unchanged."""
    th = np.where(r < lim, r, lim)
    for _ in range(steps):
        th = th - (f_poly(k, th) - r) / fp_poly(k, th)
        th = np.where(th < 0.0, F64(0.0), th)
        th = np.where(th > lim, lim, th)
    return th


def root(cam, r, steps=NEWTON_STEPS, h=None):
    """theta of r (float64 array); r > r_lim or NaN: theta = r."""
    h = h or host_constants(cam)
    r = np.asarray(r, F64)
    with np.errstate(all="ignore"):
        th = newton(ks(cam), h["theta_lim"], r, steps)
        return np.where(r <= h["r_lim"], th, r)


def fell_back(cam, r, h=None):
    h = h or host_constants(cam)
    return ~(np.asarray(r, F64) <= h["r_lim"])


# ---- sin and cos.  The reduction's constants are e_rem_pio2.c's (invpio2, pio2_1, pio2_2, pio2_2t), the kernels' coefficients
# k_sin.c's S1 .. S6 and k_cos.c's C1 .. C6 of fdlibm 5.3 (Sun Microsystems, 1993; the text FreeBSD's msun carries): public, and the
# minimax coefficients most libms share.  n stays a double throughout: nothing that can be NaN, infinite or huge becomes an integer.
INVPIO2 = F64(6.36619772367581382433e-01)
PIO2_1 = F64(1.57079632673412561417e+00)   # the first 33 bits of pi / 2
PIO2_2 = F64(6.07710050630396597660e-11)   # the next 33
PIO2_2T = F64(2.02226624879595063154e-21)  # pi / 2 - (PIO2_1 + PIO2_2)
S1, S2, S3 = F64(-1.66666666666666324348e-01), F64(8.33333333332248946124e-03), F64(-1.98412698298579493134e-04)
S4, S5, S6 = F64(2.75573137070700676789e-06), F64(-2.50507602534068634195e-08), F64(1.58969099521155010221e-10)
C1, C2, C3 = F64(4.16666666666666019037e-02), F64(-1.38888888888741095749e-03), F64(2.48015872894767294178e-05)
C4, C5, C6 = F64(-2.75573143513906633035e-07), F64(2.08757232129817482790e-09), F64(-1.13596475577881948265e-11)


def sincos(th):
    """(sin theta, cos theta).  Accurate to about an ulp while n PIO2_1 and n PIO2_2 are exact (n < 2^20); beyond, only the same bits
    on every side."""
    th = np.asarray(th, F64)
    with np.errstate(all="ignore"):
        n = np.floor(th * INVPIO2 + F64(0.5))
        y = ((th - n * PIO2_1) - n * PIO2_2) - n * PIO2_2T
        q = n - F64(4.0) * np.floor(n / F64(4.0))
        z = y * y
        s = y + (z * y) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))))
        c = F64(1.0) - (F64(0.5) * z - z * (z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))))
        swap = (q == 1.0) | (q == 3.0)
        sn, cn = np.where(swap, c, s), np.where(swap, s, c)
        sn = np.where((q == 2.0) | (q == 3.0), -sn, sn)
        cn = np.where((q == 1.0) | (q == 2.0), -cn, cn)
    return sn, cn


# ---- the lift
def plane(cam, px, h=None):
    """(x, y, r) of pixels px [..., 2] float32."""
    h = h or host_constants(cam)
    px = np.asarray(px, np.float32)
    with np.errstate(all="ignore"):
        x = h["inv11"] * px[..., 0].astype(F64) + h["inv13"]
        y = h["inv22"] * px[..., 1].astype(F64) + h["inv23"]
        return x, y, np.sqrt(x * x + y * y)


def lift(cam, px):
    """px [..., 2] float32 -> P [..., 3] float64."""
    h = host_constants(cam)
    x, y, _ = plane(cam, px, h)
    return lift_plane(cam, x, y, h)


def lift_plane(cam, x, y, h=None):
    """The lift behind the normalised plane: x, y float64 -> P [..., 3]."""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        s, c = sincos(root(cam, r, h=h))
        tiny = r < 1e-10  # :722-725
        cphi, sphi = np.where(tiny, F64(1.0), x / r), np.where(tiny, F64(0.0), y / r)
        return np.stack([s * cphi, s * sphi, c], axis=-1)


norm = tr.norm


def bearings(cam, px):
    P = lift(cam, px)
    with np.errstate(all="ignore"):
        return P / norm(P)[..., None]


def project(cam, P):
    """spaceToPlane of rays P [N, 3] (only the test inputs are made with it)."""
    return synth.camera_space_to_plane(cam, P)


# ---- the argument checks (track_plan.h); True: refused
CHECKED = ("cx", "cy", "fx", "fy", "k2", "k3", "k4", "k5")


def common_check(cam, N):
    if cam is None:
        return True
    if cam.get("model", 0) != CAM_KANNALA_BRANDT:
        return cr.common_check(cam, N)
    if not all(np.isfinite(cam[k]) for k in CHECKED):
        return True
    if cam["fx"] == 0.0 or cam["fy"] == 0.0:
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
    """track_ref.Undistort (the insert-once map and the time) with this file's lift; the text behind the lift is camera_ref's."""

    def __call__(self, cam, pts, ids, time):
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


def size_of(cam):
    for name, c in CAMERAS.items():
        if all(c[k] == cam[k] for k in CHECKED):
            return SIZES[name]
    raise KeyError("size_of: a camera of CAMERAS")


def make_matches(seed, cam, N, noise_px=1.0, outliers=0.2, size=None):
    """camera_ref.make_matches for a camera of this file and its own image size: a rigid two-view motion of points in front of the
    camera, seen through it, with noise on both pixels and a share of gross outliers."""
    W, H = size or size_of(cam)
    lo, hi = [MARGIN, MARGIN], [W - 1 - MARGIN, H - 1 - MARGIN]
    rng = np.random.default_rng([seed, 4099])
    R = gen.rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0.5, 6.0)))
    d = rng.normal(size=3)
    t = rng.uniform(0.05, 0.5) * d / np.linalg.norm(d)
    cur, forw = np.zeros((0, 2)), np.zeros((0, 2))
    while len(cur) < N:
        px = rng.uniform(lo, hi, (2 * N, 2))
        ray = synth.camera_lift(cam, px)
        X = ray / np.linalg.norm(ray, axis=1, keepdims=True) * rng.uniform(2.0, 12.0, (2 * N, 1))
        Xr = X @ R.T + t
        q = project(cam, Xr)
        qq = np.nan_to_num(q)
        ok = np.isfinite(q).all(axis=1) & (qq[:, 0] >= lo[0]) & (qq[:, 0] <= hi[0]) & (qq[:, 1] >= lo[1]) & (qq[:, 1] <= hi[1])
        cur, forw = np.vstack([cur, project(cam, X)[ok]]), np.vstack([forw, q[ok]])
    cur = cur[:N] + rng.normal(0.0, noise_px, (N, 2))
    forw = forw[:N] + rng.normal(0.0, noise_px, (N, 2))
    bad = rng.random(N) < outliers
    forw[bad] = rng.uniform(lo, hi, (int(bad.sum()), 2))
    top = np.array([W - 1.0, H - 1.0])
    return np.clip(cur, 0.0, top).astype(np.float32), np.clip(forw, 0.0, top).astype(np.float32)


make_samples = tr.make_samples
small = cr.small


def cone(rng, n, cam, size):
    """Unit rays whose pixels are inside the image: the lift of uniform pixels."""
    W, H = size
    px = rng.uniform([3 * MARGIN, 3 * MARGIN], [W - 1 - 3 * MARGIN, H - 1 - 3 * MARGIN], (n, 2))
    ray = synth.camera_lift(cam, px)
    return ray / np.linalg.norm(ray, axis=1, keepdims=True)


def undistort_sequence(seed, cam, calls=4, N=40, size=None):
    """camera_ref.undistort_sequence for a camera of this file: ids that stay, vanish, arrive as -1 and are numbered afterwards, a
    duplicate."""
    size = size or size_of(cam)
    rng = np.random.default_rng([seed, 17])
    ids = np.arange(N, dtype=np.int32)
    nxt, seq = N, []
    P = cone(rng, N, cam, size)
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
        P = np.concatenate([P[keep], cone(rng, new, cam, size)])
        ids = np.concatenate([ids[keep], np.full(new, -1, np.int32)])
    return seq


KEYS = ("model", "cx", "cy", "fx", "fy", "k2", "k3", "k4", "k5")


def cam_vector(cam):
    return np.array([cam[k] for k in KEYS], np.float64)


def cam_from_vector(v):
    cam = dict(zip(KEYS, (float(x) for x in v)))
    cam["model"] = int(v[0])
    return cam


# name: (camera, seed, N, S)
CASES = {
    "tum_40": ("TUM", 11, 40, 100),
    "cla_40": ("CLA", 12, 40, 100),
    "rsfish_40": ("RSFISH", 13, 40, 100),
    "kb_k5_0_40": ("KB_K5_0", 14, 40, 100),
    "kb_k45_0_40": ("KB_K45_0", 15, 40, 100),
    "kb_ideal_40": ("KB_IDEAL", 16, 40, 100),
    "tum_8": ("TUM", 17, 8, 4),
    "cla_7": ("CLA", 18, 7, 4),
}


def make_case(name):
    cam_name, seed, N, S = CASES[name]
    cam = CAMERAS[cam_name]
    cur, forw = make_matches(seed, cam, N, size=SIZES[cam_name], **small(N))
    return cam, cur, forw, make_samples(seed + 500, max(N, 8), S) % max(N, 1)
