"""LFVT traces (host/replay.h): the ROS-free recording of the two topics estimator_node.cpp consumes, a writer / reader,
and a seeded synthetic recording (a tracker's view of a static point cloud along synth.Scene's trajectory).

Plumbing for tests and tools: it produces INPUTS for Estimator::processIMU / processImage and the
ground truth the ATE tool compares against."""
import struct

import numpy as np

from . import abi, synth

MAGIC = b"LFVT"
REC_IMU, REC_FEATURES, REC_BOOTSTRAP, REC_TRUTH, REC_RESTART, REC_RELO, REC_SFM, REC_STRUCTURE, REC_RELATIVE = 1, 2, 3, 4, 5, 6, 7, 8, 9
REC_IMAGE = 10


class TraceWriter:
    def __init__(self, path):
        self.f = open(path, "wb")
        self.f.write(MAGIC + struct.pack("<I", 1))

    def _rec(self, kind, payload):
        self.f.write(struct.pack("<II", kind, len(payload)) + payload)

    def imu(self, t, acc, gyr):
        self._rec(REC_IMU, struct.pack("<7d", t, *acc, *gyr))

    def features(self, t, ids, xyz, u, v, vel):
        """One sensor_msgs/PointCloud of the tracker: points (float32 bearings) + channels id, u, v, vx, vy, vz (float32)."""
        n = len(ids)
        a = np.zeros((n, 9), dtype="<f4")
        a[:, 0:3] = xyz
        a[:, 3] = np.asarray(ids, dtype=np.float64) * 1 + 0  # id * NUM_OF_CAM + cam, NUM_OF_CAM = 1
        a[:, 4], a[:, 5] = u, v
        a[:, 6:9] = vel
        self._rec(REC_FEATURES, struct.pack("<dI", t, n) + a.tobytes())

    def bootstrap(self, Ps, Rs, Vs, Bas, Bgs, g, tic, ric, td, stamp=None):
        """stamp: Headers[WINDOW_SIZE] at the moment initialStructure() returned true — the record then belongs to the image
        with that stamp (a recording with reboots needs it); without it the record is taken at the first full window."""
        d = np.concatenate([np.ravel(Ps), np.ravel(Rs), np.ravel(Vs), np.ravel(Bas), np.ravel(Bgs), np.ravel(g), np.ravel(tic),
                            np.ravel(ric), [td]] + ([[stamp]] if stamp is not None else [])).astype("<f8")
        assert d.size == 11 * 21 + 3 + 13 + (stamp is not None)
        self._rec(REC_BOOTSTRAP, d.tobytes())

    def bootstrap_payload(self, payload):
        """A type-3 payload as the node's dump hook published it (247 or 248 doubles)."""
        d = np.asarray(payload, dtype="<f8")
        assert d.size in (247, 248)
        self._rec(REC_BOOTSTRAP, d.tobytes())

    def restart(self, t=None):
        """std_msgs/Bool(true) on the tracker's restart topic (restart_callback, estimator_node.cpp:187-204)."""
        self._rec(REC_RESTART, struct.pack("<d", t) if t is not None else b"")

    def relo(self, stamp, index, relo_t, relo_q_xyzw, match_points):
        """A /pose_graph/match_points message: stamp, frame index, relo_t[3], relo_q[4] (x y z w), K x (x, y, id)."""
        mp = np.asarray(match_points, dtype=np.float64).reshape(-1, 3)
        self._rec(REC_RELO, np.concatenate([[stamp, index], np.ravel(relo_t), np.ravel(relo_q_xyzw), [len(mp)], mp.ravel()]).astype("<f8").tobytes())

    def sfm(self, stamp, stamps, R, T):
        """An SfM result (type 7): stamp of the image it belongs to (Headers[WINDOW_SIZE]), then per frame of all_image_frame its
        stamp, ImageFrame::R [3, 3] (body rotation in the SfM frame) and ImageFrame::T [3] (camera position there, unscaled)."""
        stamps, R, T = np.asarray(stamps, np.float64).reshape(-1), np.asarray(R, np.float64).reshape(-1, 9), np.asarray(T, np.float64).reshape(-1, 3)
        assert len(stamps) == len(R) == len(T)
        body = np.concatenate([stamps[:, None], R, T], axis=1).astype("<f8")
        self._rec(REC_SFM, struct.pack("<dI", stamp, len(stamps)) + body.tobytes())

    def structure(self, stamp, stamps, Q, T, ids, xyz):
        """An SfM structure (type 8): stamp of the image it belongs to (Headers[WINDOW_SIZE]), then what GlobalSFM::construct() returns:
        per keyframe of the window its stamp, Q [4] (w x y z) and T [3] (camera rotation and position in the SfM frame, unscaled),
        and sfm_tracked_points as (id, xyz)."""
        stamps, Q, T = np.asarray(stamps, np.float64).reshape(-1), np.asarray(Q, np.float64).reshape(-1, 4), np.asarray(T, np.float64).reshape(-1, 3)
        ids, xyz = np.asarray(ids, np.float64).reshape(-1), np.asarray(xyz, np.float64).reshape(-1, 3)
        assert len(stamps) == len(Q) == len(T) and len(ids) == len(xyz)
        kf = np.concatenate([stamps[:, None], Q, T], axis=1).astype("<f8")
        pt = np.concatenate([ids[:, None], xyz], axis=1).astype("<f8")
        self._rec(REC_STRUCTURE, struct.pack("<dII", stamp, len(stamps), len(ids)) + kf.tobytes() + pt.tobytes())

    def relative_pose(self, stamp, l, R, T):
        """A relative pose (type 9): stamp of the image it belongs to (Headers[WINDOW_SIZE]), then what relativePose() returns: l,
        relative_R [3, 3] and relative_T [3] (the rotation and unit-norm position of the newest camera in the frame of camera l)."""
        self._rec(REC_RELATIVE, struct.pack("<di", stamp, int(l)) + np.concatenate([np.ravel(R), np.ravel(T)]).astype("<f8").tobytes())

    def truth(self, t, p, q_xyzw):
        self._rec(REC_TRUTH, struct.pack("<8d", t, *p, *q_xyzw))

    def image(self, t, img, step=None, encoding=0, width=None):
        """One sensor_msgs/Image (type 10).  encoding 0 (mono8): img [height, width] uint8; step: bytes per row in the record (default:
        width; larger: rows padded with zeros, as a driver with aligned rows sends them).  Another encoding (abi.IMG_*): img is the
        message's rows as they are, [height, step] uint8 with `width` pixels in each (padding included; step is the array's)."""
        if encoding != 0:
            a = np.ascontiguousarray(img, dtype=np.uint8)
            h, step = a.shape
            assert width is not None and step >= width * abi.IMG_BPP[encoding]
            self._rec(REC_IMAGE, struct.pack("<dIIII", t, width, h, step, encoding) + a.tobytes())
            return
        a = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = a.shape
        step = w if step is None else int(step)
        assert step >= w
        if step != w:
            a = np.concatenate([a, np.zeros((h, step - w), np.uint8)], axis=1)
        self._rec(REC_IMAGE, struct.pack("<dIIII", t, w, h, step, 0) + a.tobytes())

    def close(self):
        self.f.close()


def read_trace(path):
    """-> dict(imu [n,7], images [(t, array[n,9] float32)], bootstrap array or None, truth [n,8], raw_images [(t, array)],
    raw_steps, raw_encodings, restart_stamps [stamp or None], order [record types]).  A raw image is [h, w] uint8 (mono8), [h, w, C]
    uint8 in the record's channel order (the colour encodings) or [h, w] uint16 (mono16, either byte order, as values)."""
    out = dict(imu=[], images=[], raw_images=[], raw_steps=[], raw_encodings=[], restart_stamps=[], bootstrap=None, bootstraps=[], restarts=[], truth=[], relos=[], sfms=[], structures=[], relatives=[], order=[])
    with open(path, "rb") as f:
        head = f.read(8)
        assert head[:4] == MAGIC and struct.unpack("<I", head[4:])[0] == 1
        while True:
            h = f.read(8)
            if len(h) < 8:
                break
            kind, nbytes = struct.unpack("<II", h)
            p = f.read(nbytes)
            out["order"].append(kind)
            if kind == REC_IMU:
                out["imu"].append(struct.unpack("<7d", p))
            elif kind == REC_FEATURES:
                t, n = struct.unpack("<dI", p[:12])
                out["images"].append((t, np.frombuffer(p[12:], dtype="<f4").reshape(n, 9).copy()))
            elif kind == REC_BOOTSTRAP:
                out["bootstraps"].append(np.frombuffer(p, dtype="<f8").copy())
                if out["bootstrap"] is None:
                    out["bootstrap"] = out["bootstraps"][0]
            elif kind == REC_RESTART:
                out["restarts"].append(len(out["images"]))
                out["restart_stamps"].append(struct.unpack("<d", p)[0] if len(p) == 8 else None)
            elif kind == REC_RELO:
                d = np.frombuffer(p, dtype="<f8")
                out["relos"].append(dict(at_image=len(out["images"]), stamp=float(d[0]), index=int(d[1]), relo_t=d[2:5].copy(),
                                         relo_q=d[5:9].copy(), match_points=d[10:].reshape(-1, 3).copy()))
            elif kind == REC_SFM:
                stamp, n = struct.unpack("<dI", p[:12])
                body = np.frombuffer(p[12:], dtype="<f8").reshape(n, 13)
                out["sfms"].append(dict(at_image=len(out["images"]), stamp=stamp, stamps=body[:, 0].copy(), R=body[:, 1:10].reshape(n, 3, 3).copy(),
                                        T=body[:, 10:13].copy()))
            elif kind == REC_STRUCTURE:
                stamp, K, P = struct.unpack("<dII", p[:16])
                kf = np.frombuffer(p[16:16 + 64 * K], dtype="<f8").reshape(K, 8)
                pt = np.frombuffer(p[16 + 64 * K:], dtype="<f8").reshape(P, 4)
                out["structures"].append(dict(at_image=len(out["images"]), stamp=stamp, stamps=kf[:, 0].copy(), Q=kf[:, 1:5].copy(), T=kf[:, 5:8].copy(),
                                              ids=pt[:, 0].astype(np.int64), xyz=pt[:, 1:4].copy()))
            elif kind == REC_RELATIVE:
                stamp, l = struct.unpack("<di", p[:12])
                d = np.frombuffer(p[12:], dtype="<f8")
                out["relatives"].append(dict(at_image=len(out["images"]), stamp=stamp, l=l, R=d[:9].reshape(3, 3).copy(), T=d[9:12].copy()))
            elif kind == REC_TRUTH:
                out["truth"].append(struct.unpack("<8d", p))
            elif kind == REC_IMAGE:
                t, w, h, step, enc = struct.unpack("<dIIII", p[:24])
                assert enc in abi.IMG_BPP and len(p) == 24 + h * step
                bpp = abi.IMG_BPP[enc]
                px = np.frombuffer(p[24:], dtype=np.uint8).reshape(h, step)[:, :w * bpp].reshape(h, w, bpp)
                if enc in (abi.IMG_MONO16, abi.IMG_MONO16_BE):
                    lo, hi = (0, 1) if enc == abi.IMG_MONO16 else (1, 0)
                    img = px[:, :, lo].astype(np.uint16) | (px[:, :, hi].astype(np.uint16) << 8)
                else:
                    img = px[:, :, 0].copy() if bpp == 1 else px.copy()
                out["raw_images"].append((t, img))
                out["raw_steps"].append(step)
                out["raw_encodings"].append(enc)
    out["imu"] = np.array(out["imu"]).reshape(-1, 7)
    out["truth"] = np.array(out["truth"]).reshape(-1, 8)
    return out


def make_stream(path, seed=0, n_frames=40, n_points=600, max_cnt=150, cam_offset=0.0023, pixel_noise=1.0, boot_noise=(0.02, 0.5),
                restart_at=None, spike_at=None, spike=2.0e4, frame_dt=None, camera="sphere", w_scale=1.0):
    """Write a synthetic recording of `n_frames` images at 10 Hz with 200 Hz IMU and return what was written.

    w_scale: factor on the trajectory's angular rate (default 1.0, about 0.3 rad/s: the recording every other test uses, bit for
    bit); the online extrinsic calibration (ESTIMATE_EXTRINSIC == 2) needs more rotation than that to finish within a test.
    frame_dt: seconds between images (default synth.KF_DT = 0.1; PALVIO's camera runs at 15 Hz: 1 / 15 — README.md:76,193).
    camera = "ocam": every bearing goes through the reference's camera model like a tracked corner does — projected to a pixel by
    the inverse polynomial, disturbed by `pixel_noise` pixels, lifted back by the polynomial (ScaramuzzaCamera.cc:623-674 with the
    intrinsics of README.md:85-118; synth.ocam_*), u / v are that pixel; "sphere": noise of pixel_noise / 160 rad on the sphere.

    A static cloud of `n_points` points in a 2-12 m shell is seen through the 40-120 deg annulus; a point is tracked over
    a random span of frames and comes back under a new id afterwards, at most `max_cnt` features per image (longest
    tracks first, like the tracker's mask).  Image k is exposed at t = 0.1 k + cam_offset on the IMU clock and stamped
    t - TD0, so the estimator interpolates the IMU at image time (estimator_node.cpp:240-258).  The bootstrap record is
    the truth of the first 11 frames (+) N(0, boot_noise[0] m / boot_noise[1] deg), zero accelerometer bias.

    Reboots mid-recording (estimator.cpp:196-204, estimator_node.cpp:187-204): `restart_at = k` puts a restart message in
    front of image k; `spike_at = k` adds `spike` m/s^2 to one accelerometer sample just before image k, which throws the
    window far enough for failureDetection() to reboot the estimator while it processes that image.  Either way the
    estimator refills its window with the next ten images and a STAMPED bootstrap record — what the node's dump hook
    writes when initialStructure() succeeds again — follows for the eleventh."""
    fdt = synth.KF_DT if frame_dt is None else float(frame_dt)
    scene = synth.Scene(seed, n_total=n_frames + 2 if frame_dt is None else int(np.ceil(n_frames * fdt / synth.KF_DT)) + 3, w_scale=w_scale)
    rng = np.random.default_rng([seed, 104729])
    traj = scene.traj
    # world points and their visibility spans
    d = rng.normal(size=(n_points, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Xw = d * rng.uniform(2.0, 12.0, size=(n_points, 1))
    spans = []  # per point: list of (first, last, id)
    next_id = 0
    for p in range(n_points):
        f, s = int(rng.integers(-10, 5)), []
        while f < n_frames:
            L = int(rng.integers(3, 26))
            s.append((f, f + L - 1, next_id))
            next_id += 1
            f += L + int(rng.integers(1, 8))
        spans.append(s)

    def cam_pose(t):
        return traj.pos(t), traj.R_at(t)

    def bearings(t):
        P, R = cam_pose(t)
        Xb = (Xw - P) @ R            # R^T (X - P)
        Xc = (Xb - synth.TIC) @ synth.RIC
        return Xc / np.linalg.norm(Xc, axis=1, keepdims=True)

    w = TraceWriter(path)
    truth, images, flags = [], [], []
    boots_due = {}  # image index -> first frame of the window the bootstrap record describes
    if restart_at is not None:
        boots_due[restart_at + abi.WINDOW_SIZE] = restart_at
    if spike_at is not None:
        boots_due[spike_at + 1 + abi.WINDOW_SIZE] = spike_at + 1

    def boot_record(first, stamp=None):
        Ps, Rs, Vs = [], [], []
        for j in range(first, first + abi.NUM_FRAMES):
            tj = fdt * j + cam_offset
            Pj, Rj = cam_pose(tj)
            Ps.append(Pj + rng.normal(0, boot_noise[0], 3))
            Rs.append(Rj @ synth.exp_so3(rng.normal(0, np.deg2rad(boot_noise[1]), 3)))
            Vs.append(traj.vel(tj) + rng.normal(0, 0.02, 3))
        Bgs = np.tile(scene.bg + rng.normal(0, 0.0005, 3), (abi.NUM_FRAMES, 1))
        b = dict(Ps=np.array(Ps), Rs=np.array(Rs), Vs=np.array(Vs), Bas=np.zeros((abi.NUM_FRAMES, 3)), Bgs=Bgs,
                 g=np.array([0.0, 0.0, synth.G_NORM]), tic=synth.TIC, ric=synth.RIC, td=synth.TD0)
        w.bootstrap(stamp=stamp, **b)
        return b

    t_imu = traj.t
    k_imu = 0
    # the spans as arrays (one row per track): a frame's candidates are the tracks alive in it whose point is inside the annulus,
    # longest-seen first (the tracker's mask), ties by id
    sp_f0 = np.array([f0 for s_ in spans for (f0, f1, fid) in s_], dtype=np.int64)
    sp_f1 = np.array([f1 for s_ in spans for (f0, f1, fid) in s_], dtype=np.int64)
    sp_id = np.array([fid for s_ in spans for (f0, f1, fid) in s_], dtype=np.int64)
    sp_pt = np.array([p for p, s_ in enumerate(spans) for _ in s_], dtype=np.int64)
    seen_at = np.full(next_id, -1, dtype=np.int64)
    for k in range(n_frames):
        t_img = fdt * k + cam_offset
        # IMU messages up to and including the first one after the image (arrival order)
        if restart_at is not None and k == restart_at:
            w.restart(fdt * k)
        while k_imu < len(t_imu) and t_imu[k_imu] <= t_img + synth.IMU_DT:
            acc = scene.acc_m[k_imu]
            if spike_at is not None and k == spike_at and abs(t_imu[k_imu] - (t_img - 4 * synth.IMU_DT)) < 0.5 * synth.IMU_DT:
                acc = acc + np.array([spike, 0.0, 0.0])
            w.imu(t_imu[k_imu], acc, scene.gyr_m[k_imu])
            k_imu += 1
        b = bearings(t_img)
        b_prev = bearings(t_img - fdt) if t_img - fdt >= 0 else b
        ang = np.degrees(np.arccos(np.clip(b[:, 2], -1, 1)))
        vis = (ang >= 40.0) & (ang <= 120.0)
        alive = np.nonzero((sp_f0 <= k) & (k <= sp_f1) & vis[sp_pt])[0]
        fresh = alive[seen_at[sp_id[alive]] < 0]
        seen_at[sp_id[fresh]] = k
        order = np.lexsort((sp_pt[alive], sp_id[alive], seen_at[sp_id[alive]]))[:max_cnt]
        alive = alive[order]
        ids, pts = sp_id[alive].copy(), sp_pt[alive].copy()
        bb = b[pts]
        if camera == "ocam":
            px = synth.ocam_space_to_plane(bb) + rng.normal(0, pixel_noise, size=(len(pts), 2))
            ray = synth.ocam_lift_projective(px)
            xyz = synth._bearing_f32(ray / np.linalg.norm(ray, axis=1, keepdims=True))
            now, prev = synth.ocam_lift_projective(synth.ocam_space_to_plane(bb)), synth.ocam_lift_projective(synth.ocam_space_to_plane(b_prev[pts]))
            vel = (now / np.linalg.norm(now, axis=1, keepdims=True) - prev / np.linalg.norm(prev, axis=1, keepdims=True)) / fdt
            u, v = px[:, 0], px[:, 1]
        else:
            noise = rng.normal(0, pixel_noise / 160.0, size=bb.shape)
            noise -= bb * np.sum(noise * bb, axis=1, keepdims=True)
            xyz = synth._bearing_f32(bb + noise)
            vel = (bb - b_prev[pts]) / fdt
            u = 640.0 + 400.0 * np.arctan2(bb[:, 1], bb[:, 0]) / np.pi
            v = 480.0 + 380.0 * np.cos(np.arccos(np.clip(bb[:, 2], -1, 1)))
        vel[seen_at[ids] == k] = 0.0  # a new corner has no optical flow yet
        stamp = t_img - synth.TD0
        w.features(stamp, ids, xyz, u, v, vel)
        P, R = cam_pose(t_img)
        q = synth.R_to_q(R)  # [w x y z]
        w.truth(stamp, P, [q[1], q[2], q[3], q[0]])
        truth.append((stamp, P, R, traj.vel(t_img)))
        images.append((stamp, ids, xyz.copy(), np.stack([u, v], 1), vel.astype(np.float32).astype(np.float64)))
        if k == abi.WINDOW_SIZE - 1:  # before the 11th image arrives: what initialStructure() would have produced
            boot = boot_record(0)
        if k in boots_due:  # the estimator has refilled its window after a reboot: the hook's record for THIS image
            boot_record(boots_due[k], stamp=stamp)
    w.close()
    return dict(scene=scene, truth=truth, images=images, bootstrap=boot, n_ids=next_id, Xw=Xw, id_point=sp_pt[np.argsort(sp_id)])


def image_camera(s):
    """The PAL camera (synth.OCAM_*) for an image `s` times smaller, 1280 / s x 960 / s, as a dict for Engine.camera: the polynomial
    in pixels of the small image, z' (phi') = z (s phi') / s, the centre divided by s.  -> (camera, width, height, annulus) with
    annulus = (center_x, center_y, max_r, min_r): the pixel radii of 120 and 40 degrees from the axis, the window every recording
    of this module looks through."""
    s = float(s)
    cam = dict(cx=synth.OCAM_CX / s, cy=synth.OCAM_CY / s, c=1.0, d=0.0, e=0.0, poly=tuple(c * s ** i / s for i, c in enumerate(synth.OCAM_POLY)))
    rho = [sum(c * np.deg2rad(a - 90.0) ** i for i, c in enumerate(synth.OCAM_INV)) / s for a in (120.0, 40.0)]
    # (three pixels inside the window's rims: a corner's response looks at its 3 x 3 neighbours' 3 x 3 gradients, and the rim is an edge)
    return cam, int(round(synth.OCAM_W / s)), int(round(synth.OCAM_H / s)), (cam["cx"], cam["cy"], float(rho[0]) - 3.0, float(rho[1]) + 3.0)


def make_image_stream(path, seed=0, n_frames=36, scale=4, cam_offset=0.0023, boot_noise=(0.02, 0.5), frame_dt=None, box=(2.5, 3.5, 2.0), waves=80,
                      wavelength=(0.25, 2.5), contrast=40.0, camera=None):
    """make_stream's scene, trajectory, IMU, truth and clock convention with rendered IMAGES (record type 10) in place of the feature
    messages: `n_frames` images of 1280 / scale x 960 / scale pixels through image_camera(scale).  Image k is exposed at
    frame_dt k + cam_offset on the IMU clock and stamped that minus TD0.  Every pixel is lifted to its ray, rotated into the world
    and intersected with the INSIDE of the box |x| <= box[0], |y| <= box[1], |z| <= box[2] (metres, around the trajectory, which stays
    within 0.6 m of the origin): six walls at different distances, not one plane, on which the eight-point fit of rejectWithF would
    be degenerate.  The texture is a seeded sum of `waves` sinusoids in SPACE (wavelengths uniform in `wavelength` metres, amplitude
    proportional to the wavelength, standard deviation `contrast` grey levels around 127.5), evaluated where the ray hits the wall,
    so it has no seams at the edges.  Pixels outside the 40-120 degree annulus are black; the matching base mask is the annulus of
    image_camera.
    camera = (camera dict, width, height): a PINHOLE, MEI or KANNALA_BRANDT camera (Engine.camera) in place of image_camera(scale), which `scale`
    then does not touch.  The pixels' rays are synth.camera_lift's, every pixel with a finite ray is lit, and the base mask is all
    255: the returned annulus is None and `mask` [height, width] is that mask.

    The bootstrap record is the truth (+ boot_noise, as make_stream) of the window of the first eleven PUBLISHED messages, stamped
    with the last of them.  At 10 Hz with FREQ = 10 the node drops image 0, publishes every later image and skips the first
    publication (image 1): the window is images 2 .. 12, and the record stands in front of image 12.
    -> dict(scene, truth [(stamp, P, R, V)], stamps, camera, annulus, width, height, bootstrap, first_window)."""
    fdt = synth.KF_DT if frame_dt is None else float(frame_dt)
    scene = synth.Scene(seed, n_total=n_frames + 2 if frame_dt is None else int(np.ceil(n_frames * fdt / synth.KF_DT)) + 3)
    rng = np.random.default_rng([seed, 15485863])
    traj = scene.traj
    if camera is None:
        cam, W, H, annulus = image_camera(scale)
    else:
        (cam, W, H), annulus = camera, None
    # the texture
    lam = rng.uniform(wavelength[0], wavelength[1], waves)
    kdir = rng.normal(size=(waves, 3))
    kvec = kdir / np.linalg.norm(kdir, axis=1, keepdims=True) * (2 * np.pi / lam)[:, None]
    ph = rng.uniform(0, 2 * np.pi, waves)
    amp = lam * (contrast / np.sqrt(0.5 * (lam * lam).sum()))
    # the rays of the pixels in the camera frame
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    if camera is None:
        x, y = u - cam["cx"], v - cam["cy"]
        phi = np.hypot(x, y)
        z = sum(c * phi ** i for i, c in enumerate(cam["poly"]))
        ray = np.stack([x, y, -z], axis=-1)
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        ang = np.degrees(np.arccos(np.clip(ray[..., 2], -1, 1)))
        lit = (ang >= 40.0) & (ang <= 120.0)
    else:
        with np.errstate(all="ignore"):
            ray = synth.camera_lift(cam, np.stack([u, v], axis=-1))
            ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        lit = np.isfinite(ray).all(axis=-1)
    rays = ray[lit]  # [n, 3]
    half = np.asarray(box, np.float64)

    def render(t):
        P, R = traj.pos(t), traj.R_at(t)
        o = P + R @ synth.TIC
        d = rays @ (R @ synth.RIC).T
        with np.errstate(divide="ignore"):
            tt = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf))
        X = o + d * tt.min(axis=1)[:, None]
        g = np.zeros(len(X))
        for k in range(waves):
            g += amp[k] * np.sin(X @ kvec[k] + ph[k])
        img = np.zeros((H, W), np.uint8)
        img[lit] = np.clip(np.rint(127.5 + g), 1, 255).astype(np.uint8)
        return img

    w = TraceWriter(path)
    first_window = 2

    def boot_record(first, stamp):
        Ps, Rs, Vs = [], [], []
        for j in range(first, first + abi.NUM_FRAMES):
            tj = fdt * j + cam_offset
            Ps.append(traj.pos(tj) + rng.normal(0, boot_noise[0], 3))
            Rs.append(traj.R_at(tj) @ synth.exp_so3(rng.normal(0, np.deg2rad(boot_noise[1]), 3)))
            Vs.append(traj.vel(tj) + rng.normal(0, 0.02, 3))
        Bgs = np.tile(scene.bg + rng.normal(0, 0.0005, 3), (abi.NUM_FRAMES, 1))
        b = dict(Ps=np.array(Ps), Rs=np.array(Rs), Vs=np.array(Vs), Bas=np.zeros((abi.NUM_FRAMES, 3)), Bgs=Bgs,
                 g=np.array([0.0, 0.0, synth.G_NORM]), tic=synth.TIC, ric=synth.RIC, td=synth.TD0)
        w.bootstrap(stamp=stamp, **b)
        return b

    t_imu, k_imu, truth, stamps, boot = traj.t, 0, [], [], None
    for k in range(n_frames):
        t_img = fdt * k + cam_offset
        while k_imu < len(t_imu) and t_imu[k_imu] <= t_img + synth.IMU_DT:  # up to and including the first sample after the image
            w.imu(t_imu[k_imu], scene.acc_m[k_imu], scene.gyr_m[k_imu])
            k_imu += 1
        stamp = t_img - synth.TD0
        if k == first_window + abi.WINDOW_SIZE:
            boot = boot_record(first_window, stamp)
        w.image(stamp, render(t_img))
        P, R = traj.pos(t_img), traj.R_at(t_img)
        q = synth.R_to_q(R)  # [w x y z]
        w.truth(stamp, P, [q[1], q[2], q[3], q[0]])
        truth.append((stamp, P, R, traj.vel(t_img)))
        stamps.append(stamp)
    w.close()
    out = dict(scene=scene, truth=truth, stamps=stamps, camera=cam, annulus=annulus, width=W, height=H, bootstrap=boot, first_window=first_window)
    if camera is not None:
        out["mask"] = np.full((H, W), 255, np.uint8)
    return out


def sfm_from_truth(stamps, Ps, Rs, keyframe=0, scale=1.0, rot_noise_deg=0.0, pos_noise=0.0, seed=0, tic=None, ric=None):
    """What the vision-only half of initialStructure() would leave in all_image_frame, made from true body poses Ps [n, 3], Rs
    [n, 3, 3] of the images `stamps`: the camera poses expressed in the camera frame of image `keyframe`, positions divided by
    `scale`; ImageFrame::R = R_cl<-body (estimator.cpp:299, 355), ImageFrame::T = the camera position (:300, :356).  Optional
    noise: a rotation of rot_noise_deg (sigma per axis) on every R, a relative pos_noise on every T.  -> (stamps, R, T)."""
    tic = synth.TIC if tic is None else np.asarray(tic, float)
    ric = synth.RIC if ric is None else np.asarray(ric, float)
    rng = np.random.default_rng([seed, 7919])
    Ps, Rs = np.asarray(Ps, float).reshape(-1, 3), np.asarray(Rs, float).reshape(-1, 3, 3)
    R_wcl, p_cl = Rs[keyframe] @ ric, Ps[keyframe] + Rs[keyframe] @ tic
    R, T = np.zeros_like(Rs), np.zeros_like(Ps)
    for k in range(len(Ps)):
        R[k] = R_wcl.T @ Rs[k]
        T[k] = R_wcl.T @ (Ps[k] + Rs[k] @ tic - p_cl) / scale
        if rot_noise_deg > 0:
            R[k] = R[k] @ synth.exp_so3(rng.normal(0, np.deg2rad(rot_noise_deg), 3))
        if pos_noise > 0:
            T[k] = T[k] * (1.0 + pos_noise * rng.standard_normal(3))
    return np.asarray(stamps, float), R, T


def bootstraps_to_sfm(src, dst, keyframe=0, scale=1.0, rot_noise_deg=0.0, pos_noise=0.0, seed=0, history=40, repeat=2):
    """Copy the recording `src` to `dst` with every bootstrap record replaced by an SfM record made from the recording's ground
    truth (type 4): the record belongs to the image the bootstrap record belonged to (its stamp, or the first full window) and
    covers the last `history` images up to it — the estimator picks the frames of its list by stamp.  `repeat` records are written,
    for that image and the ones behind it: the node's hook publishes at every image whose vision-only half succeeded, and a window
    that refills after a failureDetection() reboot is full one image later than make_stream's bootstrap record assumes (the
    bootstrap path does not look at stamps, the alignment does); a record for an image the estimator is no longer initializing at is
    never handed over.  -> the list of records written for the FIRST image of each group (dicts of stamp, stamps, R, T)."""
    tr = read_trace(src)
    truth = tr["truth"]
    img_stamps = [t for t, _ in tr["images"]]
    w = TraceWriter(dst)
    written, n_img = [], 0
    with open(src, "rb") as f:
        f.read(8)
        while True:
            h = f.read(8)
            if len(h) < 8:
                break
            kind, nbytes = struct.unpack("<II", h)
            p = f.read(nbytes)
            if kind != REC_BOOTSTRAP:
                w._rec(kind, p)
                n_img += kind == REC_FEATURES
                continue
            d = np.frombuffer(p, dtype="<f8")
            stamp = float(d[247]) if d.size == 248 else img_stamps[max(n_img, abi.WINDOW_SIZE)]
            last0 = int(np.argmin(np.abs(truth[:, 0] - stamp)))
            for rep in range(repeat):
                last = last0 + rep
                if last >= len(truth):
                    break
                first = max(0, last - history + 1)
                q = truth[first:last + 1, 4:8]
                Rs = np.array([synth.q_to_R(np.array([c[3], c[0], c[1], c[2]])) for c in q])
                st, R, T = sfm_from_truth(truth[first:last + 1, 0], truth[first:last + 1, 1:4], Rs, keyframe=min(keyframe, last - first), scale=scale,
                                          rot_noise_deg=rot_noise_deg, pos_noise=pos_noise, seed=seed + len(written))
                w.sfm(float(truth[last, 0]), st, R, T)  # (where the bootstrap record stood: the replay finds a record by its stamp)
                if rep == 0:
                    written.append(dict(stamp=float(truth[last, 0]), stamps=st, R=R, T=T))
    w.close()
    return written


def structure_from_truth(stamps, Ps, Rs, ids, Xw, keyframe=0, scale=1.0, rot_noise_deg=0.0, pos_noise=0.0, point_noise=0.0, seed=0, tic=None, ric=None):
    """What GlobalSFM::construct() would return, made from true body poses Ps [K, 3], Rs [K, 3, 3] of the window's keyframes and
    the true landmark positions Xw [P, 3] (world frame): camera rotations Q (w x y z) and positions T in the camera frame of
    keyframe `keyframe`, and the landmarks there, everything divided by `scale`.  Optional noise: a rotation of rot_noise_deg
    (sigma per axis) on every Q, a relative pos_noise on every T, point_noise (relative, per coordinate) on every landmark.
    -> (stamps, Q [K, 4], T [K, 3], ids, xyz [P, 3])."""
    tic = synth.TIC if tic is None else np.asarray(tic, float)
    ric = synth.RIC if ric is None else np.asarray(ric, float)
    rng = np.random.default_rng([seed, 104723])
    Ps, Rs, Xw = np.asarray(Ps, float).reshape(-1, 3), np.asarray(Rs, float).reshape(-1, 3, 3), np.asarray(Xw, float).reshape(-1, 3)
    R_wcl, p_cl = Rs[keyframe] @ ric, Ps[keyframe] + Rs[keyframe] @ tic
    Q, T = np.zeros((len(Ps), 4)), np.zeros_like(Ps)
    for k in range(len(Ps)):
        Rk = R_wcl.T @ Rs[k] @ ric
        T[k] = R_wcl.T @ (Ps[k] + Rs[k] @ tic - p_cl) / scale
        if rot_noise_deg > 0:
            Rk = Rk @ synth.exp_so3(rng.normal(0, np.deg2rad(rot_noise_deg), 3))
        if pos_noise > 0:
            T[k] = T[k] * (1.0 + pos_noise * rng.standard_normal(3))
        Q[k] = synth.R_to_q(Rk)
    xyz = (Xw - p_cl) @ R_wcl / scale
    if point_noise > 0:
        xyz = xyz * (1.0 + point_noise * rng.standard_normal(xyz.shape))
    return np.asarray(stamps, float), Q, T, np.asarray(ids, np.int64), xyz


def relative_pose_from_truth(Ps, Rs, l, tic=None, ric=None):
    """What relativePose() is meant to return, made from true body poses Ps [K, 3], Rs [K, 3, 3] of the window's keyframes: the rotation
    of the newest camera in the frame of camera l and its position there scaled to unit norm.  -> (relative_R [3, 3], relative_T [3])."""
    tic = synth.TIC if tic is None else np.asarray(tic, float)
    ric = synth.RIC if ric is None else np.asarray(ric, float)
    Ps, Rs = np.asarray(Ps, float).reshape(-1, 3), np.asarray(Rs, float).reshape(-1, 3, 3)
    R_wcl, p_cl = Rs[l] @ ric, Ps[l] + Rs[l] @ tic
    T = R_wcl.T @ (Ps[-1] + Rs[-1] @ tic - p_cl)
    return R_wcl.T @ Rs[-1] @ ric, T / np.linalg.norm(T)


def bootstraps_to_structure(src, dst, made, keyframe=0, scale=1.0, rot_noise_deg=0.0, pos_noise=0.0, point_noise=0.0, seed=0, repeat=2,
                            skip=0):
    """Copy the recording `src` (written by make_stream, whose return value is `made`: the landmark of every feature id is needed)
    to `dst` with every bootstrap record replaced by SfM structure records made from ground truth, as bootstraps_to_sfm() does for
    type 7.  Which images are the window's keyframes is the estimator's decision (the parallax test): `made["keyframes_of"]`, if
    present, is a function stamp -> the stamps of the window's keyframes when the image `stamp` arrives; without it the eleven
    images up to the record's are taken (right for a recording whose every image is a keyframe).  The points are the landmarks of
    every feature id seen in those keyframes.  skip: the first record is written for the image `skip` images behind the bootstrap
    record's (a list with non-keyframes needs a few slides first).  -> the records written for the FIRST image of each group."""
    tr = read_trace(src)
    truth = tr["truth"]
    img_stamps = [t for t, _ in tr["images"]]
    id_point, Xw = made["id_point"], made["Xw"]
    keyframes_of = made.get("keyframes_of")
    w = TraceWriter(dst)
    written, n_img = [], 0
    with open(src, "rb") as f:
        f.read(8)
        while True:
            h = f.read(8)
            if len(h) < 8:
                break
            kind, nbytes = struct.unpack("<II", h)
            p = f.read(nbytes)
            if kind != REC_BOOTSTRAP:
                w._rec(kind, p)
                n_img += kind == REC_FEATURES
                continue
            d = np.frombuffer(p, dtype="<f8")
            stamp = float(d[247]) if d.size == 248 else img_stamps[max(n_img, abi.WINDOW_SIZE)]
            last0 = int(np.argmin(np.abs(truth[:, 0] - stamp)))
            for rep in range(skip, skip + repeat):
                last = last0 + rep
                if last >= len(truth):
                    break
                ks = keyframes_of(float(truth[last, 0])) if keyframes_of else truth[max(0, last - abi.WINDOW_SIZE):last + 1, 0]
                rows = [int(np.argmin(np.abs(truth[:, 0] - s_))) for s_ in ks]
                q = truth[rows, 4:8]
                Rs = np.array([synth.q_to_R(np.array([c[3], c[0], c[1], c[2]])) for c in q])
                seen = sorted({int(i) for r in rows for i in tr["images"][r][1][:, 3].astype(np.int64)})
                st = structure_from_truth(truth[rows, 0], truth[rows, 1:4], Rs, seen, Xw[[id_point[i] for i in seen]], keyframe=min(keyframe, len(rows) - 1),
                                          scale=scale, rot_noise_deg=rot_noise_deg, pos_noise=pos_noise, point_noise=point_noise, seed=seed + len(written))
                w.structure(float(truth[last, 0]), *st)
                if rep == skip:
                    written.append(dict(stamp=float(truth[last, 0]), stamps=st[0], Q=st[1], T=st[2], ids=st[3], xyz=st[4]))
    w.close()
    return written
