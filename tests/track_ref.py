"""numpy restatement of lfvio_track_reject / lfvio_track_undistort (include/lfvio.h): the specification of the two
steps of FeatureTracker::readImage that need the camera — rejectWithF (feature_tracker/src/feature_tracker.cpp:329-386 with
myfindFundamentalMat :266-327) and undistortedPoints (:441-504) over OCAMCamera::liftProjective (ScaramuzzaCamera.cc:623-645).

  lift, bearings   the lift in double, one rounding per operation (numpy fuses nothing), and P / n with n = sqrt((x x + y y) + z z),
                   left to right.  Eigen's own reduction may order the three terms differently and differ in the last bit; the
                   reference does not build without Eigen and OpenCV, so nobody has compared the two.
  reject           the lift, then twoview_ref.two_view's hypotheses, selection, refit and mask, and the three status cases
  Undistort        the state object of undistortedPoints: the insert-once map of the previous call and its time
  reject_check, undistort_check   the argument checks of track_plan.h, field by field
  CASES            the fixture cases of tests/golden/track_cases.npz, from seeds (tests/golden/gen_track.py writes the file)

A camera is a dict: cx, cy, c, d, e, poly [5] and, optionally, model."""
import numpy as np

import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio import synth

MAX_POINTS, MAX_SAMPLES, MIN_MATCHES, CAM_OCAM = 4096, 1024, 8, 0

PAL = dict(cx=synth.OCAM_CX, cy=synth.OCAM_CY, c=1.0, d=0.0, e=0.0, poly=synth.OCAM_POLY)
# a second camera: the affine part away from (1, 0, 0) and a centre that IS a float32 pixel, so that a pixel can sit exactly on it
SKEW = dict(cx=640.5, cy=479.25, c=1.0007, d=-0.0023, e=0.0031, poly=synth.OCAM_POLY)


# ---- the lift
def lift(cam, px):
    """px [..., 2] float32 -> P [..., 3] float64 (liftProjective, :623-645)."""
    px = np.asarray(px, np.float32)
    c, d, e = np.float64(cam["c"]), np.float64(cam["d"]), np.float64(cam["e"])
    inv_scale = np.float64(1.0) / (c - d * e)
    with np.errstate(all="ignore"):
        x = px[..., 0].astype(np.float64) - np.float64(cam["cx"])
        y = px[..., 1].astype(np.float64) - np.float64(cam["cy"])
        xa = inv_scale * (x - d * y)
        ya = inv_scale * (-e * x + c * y)
        phi = np.sqrt(xa * xa + ya * ya)
        z, p = np.zeros_like(phi), np.ones_like(phi)
        for i in range(5):
            z = z + p * np.float64(cam["poly"][i])
            p = p * phi
    return np.stack([xa, ya, -z], axis=-1)


def norm(P):
    with np.errstate(all="ignore"):
        return np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])


def bearings(cam, px):
    P = lift(cam, px)
    with np.errstate(all="ignore"):
        return P / norm(P)[..., None]


def project(cam, P):
    """spaceToPlane of rays P [N, 3] for a camera of this file: synth.ocam_space_to_plane's pixel, moved from the PAL centre through
    the affine part to the camera's own (only the test inputs are made with it)."""
    uv = synth.ocam_space_to_plane(P) - np.array([synth.OCAM_CX, synth.OCAM_CY])
    return np.stack([cam["c"] * uv[:, 0] + cam["d"] * uv[:, 1] + cam["cx"], cam["e"] * uv[:, 0] + uv[:, 1] + cam["cy"]], axis=-1)


# ---- the argument checks (track_plan.h); True: refused
def common_check(cam, N):
    return cam is None or cam.get("model", CAM_OCAM) != CAM_OCAM or N < 0 or N > MAX_POINTS


def reject_check(cam, N, have_cur, have_forw, S, samples):
    """samples: None (a null pointer) or an int array [S, 8]."""
    if common_check(cam, N):
        return True
    if N > 0 and not (have_cur and have_forw):
        return True
    if N < MIN_MATCHES:
        return False
    if S < 1 or S > MAX_SAMPLES or samples is None:
        return True
    s = np.asarray(samples).reshape(-1)[:8 * S]
    return bool(np.any((s < 0) | (s >= N)))


def undistort_check(cam, N, have_pts, have_ids, time):
    if common_check(cam, N):
        return True
    if N > 0 and not (have_pts and have_ids):
        return True
    return bool(np.isnan(time))


# ---- rejectWithF
def reject(cam, cur_pts, forw_pts, samples):
    """dict: status (0 model, 1 no model, 2 fewer than 8 matches), mask (= status[] of the call), best_sample, num_inliers,
    best_score, E (status 0), bearing_cur, bearing_forw, and twoview_ref's c1_gap / c2_margin where they exist."""
    cur, forw = np.asarray(cur_pts, np.float32).reshape(-1, 2), np.asarray(forw_pts, np.float32).reshape(-1, 2)
    N = len(cur)
    if N < MIN_MATCHES:
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


def conditions(r):
    """C1 and C2 of tests/test_two_view.py on a result of reject()."""
    return r["status"] == 0 and r["c1_gap"] > 1e-4 and r["c2_margin"] > 1e-6


# ---- undistortedPoints
class Undistort:
    """The state of undistortedPoints: prev_un_pts_map_3d (built with std::map::insert: the first occurrence of an id wins, ids as
    passed, -1 included) and prev_time."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.ids, self.p3d, self.time = np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 0.0

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
def make_matches(seed, cam, N, noise_px=1.0, outliers=0.2, centre=False):
    """A rigid two-view motion seen through the camera: (cur_pts, forw_pts) float32 [N, 2] with noise_px of Gaussian noise on both
    pixels and a share of gross outliers (forw pixels drawn anew from the annulus).  centre: point 0's cur pixel is the centre."""
    c = gen.make_case(seed, N, noise_px=0.0, outliers=0.0)
    rng = np.random.default_rng([seed, 991])
    cur = project(cam, c["bl"]) + rng.normal(0.0, noise_px, (N, 2))
    forw = project(cam, c["br"]) + rng.normal(0.0, noise_px, (N, 2))
    bad = rng.random(N) < outliers
    forw[bad] = project(cam, gen.annulus(rng, int(bad.sum()), (40.0, 120.0)))
    cur, forw = cur.astype(np.float32), forw.astype(np.float32)
    if centre:
        cur[0] = cam["cx"], cam["cy"]
    return cur, forw


def make_samples(seed, N, S):
    return gen.make_samples(seed, N, S)


# name: (camera, seed, N, S, centre)
CASES = {
    "pal_60": (PAL, 11, 60, 100, False),
    "pal_97": (PAL, 12, 97, 100, False),
    "skew_80": (SKEW, 13, 80, 100, False),
    "skew_centre_45": (SKEW, 14, 45, 100, True),
    "pal_8": (PAL, 15, 8, 4, False),
    "pal_7": (PAL, 16, 7, 4, False),
}


def make_case(name):
    cam, seed, N, S, centre = CASES[name]
    kw = dict(noise_px=0.2, outliers=0.0) if N < 30 else {}
    cur, forw = make_matches(seed, cam, N, centre=centre, **kw)
    return cam, cur, forw, make_samples(seed + 500, max(N, 8), S) % max(N, 1)


def undistort_sequence(seed, cam, calls=4, N=40):
    """A short sequence for the fixture: ids that stay, vanish, arrive as -1 and are numbered afterwards, a duplicate."""
    rng = np.random.default_rng([seed, 17])
    ids = np.arange(N, dtype=np.int32)
    nxt, seq = N, []
    P = gen.annulus(rng, N, (40.0, 120.0))
    for k in range(calls):
        P = P + rng.normal(0.0, 0.01, P.shape)
        pts = (project(cam, P) + rng.normal(0.0, 0.3, (len(P), 2))).astype(np.float32)
        call_ids = ids.copy()
        if k == 2:
            call_ids[5] = call_ids[3]  # a duplicate
        seq.append((pts, call_ids.copy(), 0.05 * k + 1.0))
        # the caller numbers the -1s, drops a few, detects new corners
        for i in range(len(ids)):
            if ids[i] == -1:
                ids[i], nxt = nxt, nxt + 1
        keep = rng.random(len(ids)) > 0.15
        new = int((~keep).sum())
        P = np.concatenate([P[keep], gen.annulus(rng, new, (40.0, 120.0))])
        ids = np.concatenate([ids[keep], np.full(new, -1, np.int32)])
    return seq


def cam_vector(cam):
    return np.array([cam.get("model", CAM_OCAM), cam["cx"], cam["cy"], cam["c"], cam["d"], cam["e"], *cam["poly"]], np.float64)


def cam_from_vector(v):
    return dict(model=int(v[0]), cx=float(v[1]), cy=float(v[2]), c=float(v[3]), d=float(v[4]), e=float(v[5]), poly=tuple(float(x) for x in v[6:11]))
