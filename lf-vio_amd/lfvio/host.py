"""ctypes driver of the host-side C++ mirror (liblfvio_host.so): Estimator / FeatureManager /
IntegrationBase with the reference's member names, optimization() re-implemented over the C-ABI."""
import ctypes as C
import os

import numpy as np

from . import abi, synth

_dp = C.POINTER(C.c_double)
HOST_LIB_PATH = os.path.join(abi.PKG_DIR, "liblfvio_host.so")


def _p(a):
    return a.ctypes.data_as(_dp)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class HostEstimator:
    def __init__(self, lib_path=None):
        """lib_path: another build of the same host sources (the test suite links one against its CPU checker); the
        default is the product build over liblfvio_hip.so, and there is no fallback if that is missing."""
        lib_path = lib_path or HOST_LIB_PATH
        if not os.path.exists(lib_path):
            raise RuntimeError(f"{lib_path} not found: run __graft_entry__.build()")
        L = C.CDLL(lib_path)
        L.lfvio_host_create.restype = C.c_void_p
        ip = C.POINTER(C.c_int)
        L.lfvio_host_destroy.argtypes = [C.c_void_p]
        L.lfvio_host_set_params.argtypes = [_dp, C.c_int, C.c_int, C.c_int]
        L.lfvio_host_set_state.argtypes = [C.c_void_p] + [_dp] * 7 + [C.c_double]
        L.lfvio_host_get_state.argtypes = [C.c_void_p] + [_dp] * 8
        L.lfvio_host_clear_features.argtypes = [C.c_void_p]
        L.lfvio_host_add_feature.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double]
        L.lfvio_host_feature_count.argtypes = [C.c_void_p]
        L.lfvio_host_get_depths.argtypes = [C.c_void_p, _dp]
        L.lfvio_host_set_imu.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp]
        L.lfvio_host_repropagate.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.lfvio_host_repropagate_window.argtypes = [C.c_void_p, _dp, _dp]
        L.lfvio_host_set_min_parallax.argtypes = [C.c_double]
        L.lfvio_host_process_imu.argtypes = [C.c_void_p, C.c_double, _dp, _dp]
        L.lfvio_host_process_image.argtypes = [C.c_void_p, C.c_double, C.c_int, ip, _dp]
        L.lfvio_host_add_feature_check_parallax.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, _dp, C.c_double]
        L.lfvio_host_set_bootstrap.argtypes = [C.c_void_p] + [_dp] * 6
        L.lfvio_host_set_running.argtypes = [C.c_void_p] + [_dp] * 4
        L.lfvio_host_clear_state.argtypes = [C.c_void_p]
        L.lfvio_host_slide_window.argtypes = [C.c_void_p]
        L.lfvio_host_failure_detection.argtypes = [C.c_void_p]
        L.lfvio_host_get_flow.argtypes = [C.c_void_p, ip]
        L.lfvio_host_get_buffers.argtypes = [C.c_void_p, _dp, ip, ip, _dp]
        L.lfvio_host_replay.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, ip]
        L.lfvio_host_decode_features.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, _dp, _dp]
        L.lfvio_host_vector2double.argtypes = [C.c_void_p]
        L.lfvio_host_double2vector.argtypes = [C.c_void_p]
        L.lfvio_host_get_para.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
        L.lfvio_host_set_para.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_double, _dp, C.c_int]
        L.lfvio_host_pack.argtypes = [C.c_void_p, C.POINTER(abi.WindowC)]
        L.lfvio_host_set_flag.argtypes = [C.c_void_p, C.c_int]
        L.lfvio_host_set_prior.argtypes = [C.c_void_p, C.POINTER(abi.Prior)]
        L.lfvio_host_get_prior.argtypes = [C.c_void_p, C.POINTER(abi.Prior)]
        L.lfvio_host_optimization.argtypes = [C.c_void_p]
        L.lfvio_host_set_fused.argtypes = [C.c_void_p, C.c_int]
        L.lfvio_host_set_device_mask.argtypes = [C.c_uint]
        L.lfvio_host_set_local_shards.argtypes = [C.c_int]
        L.lfvio_host_set_split_call.argtypes = [C.c_int]
        L.lfvio_host_collect_prior.argtypes = [C.c_void_p]
        L.lfvio_host_get_timers.argtypes = [C.c_void_p, _dp, C.c_int]
        L.lfvio_host_uses_group.argtypes = [C.c_void_p]
        L.lfvio_host_triangulate.argtypes = [C.c_void_p]
        L.lfvio_host_remove_back_shift_depth.argtypes = [C.c_void_p, _dp, _dp]
        L.lfvio_host_num_features.argtypes = [C.c_void_p]
        L.lfvio_host_list_features.argtypes = [C.c_void_p, ip, ip, ip, _dp]
        L.lfvio_host_set_depths.argtypes = [C.c_void_p, _dp, C.c_int]
        L.lfvio_host_last_iterations.argtypes = [C.c_void_p]
        L.lfvio_host_last_cost.argtypes = [C.c_void_p]
        L.lfvio_host_last_cost.restype = C.c_double
        # the image route (host/tracker_capi.cpp): the product build has it, the suite's CPU build of the estimator's sources does not
        self.has_tracker = hasattr(L, "lfvio_host_track_trace")
        if self.has_tracker:
            L.lfvio_host_track_config.argtypes = [C.POINTER(abi.CameraC), ip, _dp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]
            L.lfvio_host_track_config.restype = None
            if hasattr(L, "lfvio_host_track_expand"):
                L.lfvio_host_track_expand.argtypes = [C.POINTER(abi.ProjectorC), C.c_int, C.c_int, C.c_int, _dp]
                L.lfvio_host_track_expand.restype = None
            L.lfvio_host_track_trace.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, _dp]
            L.lfvio_host_replay_images.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, ip, _dp]
            L.lfvio_host_trace_raw_images.argtypes = [C.c_char_p, C.c_int, _dp, C.c_char_p, C.c_int]
            if hasattr(L, "lfvio_host_trace_raw_encoding"):
                L.lfvio_host_trace_raw_encoding.argtypes = [C.c_char_p]
            if hasattr(L, "lfvio_host_track_traces"):
                L.lfvio_host_track_traces.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), _dp]
                L.lfvio_host_track_traces_error.argtypes = []
                L.lfvio_host_track_traces_error.restype = C.c_char_p
        self.L = L
        self.h = L.lfvio_host_create()

    def close(self):
        if self.h:
            self.L.lfvio_host_destroy(self.h)
            self.h = None

    def load_window(self, win):
        """Feed the Estimator members the way processIMU()/processImage() would have (estimator.cpp:86-220)."""
        p = _f([synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W, win.g[2], win.tr, win.row, -1.0, synth.TD0])
        self.L.lfvio_host_set_params(_p(p), win.estimate_extrinsic, win.estimate_td, win.max_num_iterations)
        Ps = _f(win.pose[:, :3])
        Rs = _f([synth.pose_R(win.pose[f]) for f in range(11)])
        Vs, Bas, Bgs = _f(win.speed_bias[:, 0:3]), _f(win.speed_bias[:, 3:6]), _f(win.speed_bias[:, 6:9])
        tic, ric = _f(win.ex_pose[:3]), _f(synth.pose_R(win.ex_pose))
        self.L.lfvio_host_set_state(self.h, _p(Ps), _p(Rs), _p(Vs), _p(Bas), _p(Bgs), _p(tic), _p(ric), win.td)
        self.L.lfvio_host_clear_features(self.h)
        for l in range(win.N):
            o0, o1 = int(win.obs_offset[l]), int(win.obs_offset[l + 1])
            obs = np.zeros((o1 - o0, 8))
            obs[:, 0:3] = win.obs_point[o0:o1]
            obs[:, 4] = win.obs_uv_y[o0:o1]
            obs[:, 5:8] = win.obs_velocity[o0:o1]
            ctd = _f(win.obs_cur_td[o0:o1])
            self.L.lfvio_host_add_feature(self.h, l, int(win.start_frame[l]), o1 - o0, _p(_f(obs)), _p(ctd),
                                          1.0 / float(win.inv_depth[l]))
        for i, (ba, bg, a0, g0, dts, accs, gyrs) in enumerate(win.raw_imu):
            self.L.lfvio_host_set_imu(self.h, i + 1, _p(_f(a0)), _p(_f(g0)), _p(_f(ba)), _p(_f(bg)), len(dts), _p(_f(dts)),
                                      _p(_f(accs)), _p(_f(gyrs)))
        self.L.lfvio_host_set_prior(self.h, C.byref(win.prior) if win.prior is not None else None)

    # ---- control flow and trace replay
    FLOW = ("solver_flag", "marginalization_flag", "frame_count", "sum_of_back", "sum_of_front", "last_track_num", "features",
            "failure_occur")

    def clear_state(self):
        self.L.lfvio_host_clear_state(self.h)

    def set_solver_time(self, seconds):
        """SOLVER_TIME (parameters.cpp:133); <= 0 switches the wall-clock cap of the solve off."""
        self.L.lfvio_host_set_solver_time.argtypes = [C.c_double]
        self.L.lfvio_host_set_solver_time(float(seconds))

    def set_min_parallax(self, keyframe_parallax_px):
        self.L.lfvio_host_set_min_parallax(float(keyframe_parallax_px))

    def process_imu(self, dt, acc, gyr):
        self.L.lfvio_host_process_imu(self.h, float(dt), _p(_f(acc)), _p(_f(gyr)))

    @staticmethod
    def _image(ids, pts):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        pts = _f(pts).reshape(len(ids), 8)
        return ids, pts

    def process_image(self, stamp, ids, pts):
        """pts[n][8] = x y z u v vx vy vz; returns the status of the device calls inside (0 = ok)."""
        ids, pts = self._image(ids, pts)
        return self.L.lfvio_host_process_image(self.h, float(stamp), len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), _p(pts))

    def add_feature_check_parallax(self, frame_count, ids, pts, td):
        ids, pts = self._image(ids, pts)
        return bool(self.L.lfvio_host_add_feature_check_parallax(self.h, frame_count, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)),
                                                                 _p(pts), float(td)))

    def set_bootstrap(self, Ps, Rs, Vs, Bas, Bgs, g, depth_ids=None, depths=None):
        """depth_ids / depths (optional): the depths that belong to the state, by feature id — what visualInitialAlign() leaves
        beside Ps .. g (estimator.cpp:389-425); without them every track is triangulated on the state."""
        a = [_f(x) for x in (Ps, Rs, Vs, Bas, Bgs, g)]
        self.L.lfvio_host_set_bootstrap(self.h, *[_p(x) for x in a])
        if depth_ids is not None:
            ids, d = np.ascontiguousarray(depth_ids, dtype=np.int32), _f(depths)
            self.L.lfvio_host_set_bootstrap_depths.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]
            self.L.lfvio_host_set_bootstrap_depths(self.h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), _p(d))

    def set_running(self, stamps, acc_0, gyr_0, g):
        a = [_f(x) for x in (stamps, acc_0, gyr_0, g)]
        self.L.lfvio_host_set_running(self.h, *[_p(x) for x in a])

    def slide_window(self):
        self.L.lfvio_host_slide_window(self.h)

    def failure_detection(self):
        return bool(self.L.lfvio_host_failure_detection(self.h))

    def collect_prior(self):
        """Wait for the marginalization a split optimization() left running on the device; 0 or the error code."""
        return self.L.lfvio_host_collect_prior(self.h)

    def timers(self, reset=True):
        """Seconds in the device-backed steps since the last reset: optimization() up to the state, collectPrior(),
        triangulate(), reanchorDepths(), refreshSpans(); and the number of optimization() calls."""
        o = np.zeros(6)
        self.L.lfvio_host_get_timers(self.h, o.ctypes.data_as(_dp), int(reset))
        return dict(optimization=o[0], collect_prior=o[1], triangulate=o[2], reanchor=o[3], spans=o[4], calls=int(o[5]))

    def flow(self):
        o = np.zeros(8, dtype=np.int32)
        self.L.lfvio_host_get_flow(self.h, o.ctypes.data_as(C.POINTER(C.c_int)))
        return dict(zip(self.FLOW, (int(x) for x in o)))

    def buffers(self):
        st, sd = np.zeros(11), np.zeros(11)
        ns, hp = np.zeros(11, dtype=np.int32), np.zeros(11, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_get_buffers(self.h, _p(st), ns.ctypes.data_as(ip), hp.ctypes.data_as(ip), _p(sd))
        return dict(stamps=st, num_samples=ns, has_pre=hp, sum_dt=sd)

    STATS = ("images", "thrown", "keyframes", "non_keyframes", "poses", "failures", "last_status", "iterations", "restarts", "bootstraps",
             "relocalizations")

    def replay(self, trace_path, traj_path="", max_images=0):
        """-> (rc, stats dict); rc 0 ok, -2 a device call failed (stats['last_status']), -3 unreadable trace."""
        o = np.zeros(len(self.STATS), dtype=np.int32)
        rc = self.L.lfvio_host_replay(self.h, str(trace_path).encode(), str(traj_path).encode(), int(max_images),
                                      o.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, dict(zip(self.STATS, (int(x) for x in o)))

    def replay_timed(self, trace_path, traj_path="", max_images=0, cap=65536):
        """replay() with the wall-clock milliseconds the loop spent on every image it handed over -> (rc, stats, ms[n])."""
        o, ms, n = np.zeros(len(self.STATS), dtype=np.int32), np.zeros(cap), C.c_int(0)
        self.L.lfvio_host_replay_timed.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), _dp, C.c_int, C.POINTER(C.c_int)]
        rc = self.L.lfvio_host_replay_timed(self.h, str(trace_path).encode(), str(traj_path).encode(), int(max_images),
                                            o.ctypes.data_as(C.POINTER(C.c_int)), _p(ms), cap, C.byref(n))
        return rc, dict(zip(self.STATS, (int(x) for x in o))), ms[:n.value].copy()

    TRACK_STATS = ("raw_images", "dropped", "restarts", "tracked_only", "published", "rows", "tracker_ms")

    def _tracker(self):
        if not self.has_tracker:
            raise RuntimeError("this build of the host library has no image route (host/tracker_capi.cpp): use the product build")

    def track_config(self, cam, max_cnt=150, min_dist=30, freq=10, equalize=False, num_samples=100, seed=0, annulus=None, mask=None):
        """lfvio_host_track_config: the tracker of the next track_trace / replay_images.  cam: a dict as Engine.camera takes (or a
        CameraC); annulus = (center_x, center_y, max_r, min_r) or mask [height, width] uint8: the base mask; seed 0: std::random_device."""
        self._tracker()
        camc = cam if isinstance(cam, abi.CameraC) else abi.camera_c(cam)
        iv = np.array([max_cnt, min_dist, freq, int(bool(equalize)), num_samples, seed], dtype=np.uint32).view(np.int32)
        an = None if annulus is None else _f(annulus)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.L.lfvio_host_track_config(C.byref(camc), iv.ctypes.data_as(C.POINTER(C.c_int)), None if an is None else _p(an),
                                       0 if m is None else m.shape[1], 0 if m is None else m.shape[0],
                                       None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte)))

    def track_expand(self, src_cam, kind=abi.MAP_EQUIRECT, width=0, height=0, M=None):
        """lfvio_host_track_expand, BEHIND track_config: the next track_trace / replay_images tracks on the width x height image expanded
        from the records' raw images through the SOURCE camera src_cam (a dict as Engine.projector takes: an OCam camera with its
        inv_poly) — kind abi.MAP_EQUIRECT, or abi.MAP_PERSPECTIVE with M [3, 3].  track_config's camera is then the expanded image's
        (abi.CAM_EQUIRECT with fx, fy = width, height for MAP_EQUIRECT) and its mask of that size.  src_cam None: off."""
        self._tracker()
        if src_cam is None:
            self.L.lfvio_host_track_expand(None, 0, 0, 0, None)
            return
        proj, keep = abi.projector_c(src_cam)
        m = None if M is None else _f(np.asarray(M, dtype=np.float64).reshape(9))
        self.L.lfvio_host_track_expand(C.byref(proj), int(kind), int(width), int(height), None if m is None else _p(m))
        del keep

    def track_trace(self, in_path, out_path):
        """lfvio_host_track_trace: the recording with its raw images (type 10) replaced by what the tracker published for them.
        -> (rc, track stats dict); rc 0 ok, -1 cannot write, -2 a device call failed, -3 unreadable or refused trace."""
        self._tracker()
        ts = np.zeros(len(self.TRACK_STATS))
        rc = self.L.lfvio_host_track_trace(self.h, str(in_path).encode(), str(out_path).encode(), _p(ts))
        return rc, dict(zip(self.TRACK_STATS, (float(x) for x in ts)))

    def track_traces(self, in_paths, out_paths):
        """lfvio_host_track_traces: several recordings through one batched tracker call per round — round r takes the r-th raw image of
        every recording that still has one.  Every out_paths[i] is what track_trace writes for in_paths[i] alone.  -> (rc, [track stats
        dict per recording]); rc 0 ok, -1 cannot write, -2 a device call failed, -3 unreadable or refused, -4 the images of a round
        disagree in width, height, step or encoding; on anything but 0 no file is written (track_traces_error() says why)."""
        self._tracker()
        n = len(in_paths)
        assert len(out_paths) == n
        ins = (C.c_char_p * max(n, 1))(*[str(p).encode() for p in in_paths])
        outs = (C.c_char_p * max(n, 1))(*[str(p).encode() for p in out_paths])
        ts = np.zeros((max(n, 1), len(self.TRACK_STATS)))
        rc = self.L.lfvio_host_track_traces(self.h, n, ins, outs, _p(ts))
        return rc, [dict(zip(self.TRACK_STATS, (float(x) for x in row))) for row in ts[:n]]

    def track_traces_error(self):
        """Why the last track_traces failed ("" after one that did not)."""
        return self.L.lfvio_host_track_traces_error().decode()

    def replay_images(self, trace_path, traj_path="", max_images=0):
        """lfvio_host_replay_images: pixels to poses -> (rc, stats dict as replay(), track stats dict)."""
        self._tracker()
        o, ts = np.zeros(len(self.STATS), dtype=np.int32), np.zeros(len(self.TRACK_STATS))
        rc = self.L.lfvio_host_replay_images(self.h, str(trace_path).encode(), str(traj_path).encode(), int(max_images),
                                             o.ctypes.data_as(C.POINTER(C.c_int)), _p(ts))
        return rc, dict(zip(self.STATS, (int(x) for x in o))), dict(zip(self.TRACK_STATS, (float(x) for x in ts)))

    def trace_raw_images(self, trace_path, cap=4096):
        """The raw images of a trace file as the host loader keeps them -> (n or -3, array [n, 5] = stamp, width, height, step, offset
        of the pixels in the file, the loader's message where it refused)."""
        self._tracker()
        o, err = np.zeros((cap, 5)), C.create_string_buffer(256)
        n = self.L.lfvio_host_trace_raw_images(str(trace_path).encode(), cap, _p(o), err, 256)
        return n, o[:max(min(n, cap), 0)].copy(), err.value.decode()

    def trace_raw_encoding(self, trace_path):
        """The encoding (abi.IMG_*) the raw images of a trace file share, as the host loader keeps it; -1: no raw images, -3: refused."""
        self._tracker()
        return self.L.lfvio_host_trace_raw_encoding(str(trace_path).encode())

    def decode_features(self, trace_path, image_index, cap=4096):
        ids, pts, st = np.zeros(cap, dtype=np.int32), np.zeros((cap, 8)), np.zeros(1)
        n = self.L.lfvio_host_decode_features(str(trace_path).encode(), image_index, cap, ids.ctypes.data_as(C.POINTER(C.c_int)), _p(pts), _p(st))
        return float(st[0]), ids[:n], pts[:n]

    # ---- SURVEY §8f rank 3
    def repropagate_window(self, ba, bg):
        """Estimator::repropagateWindow: every pre_integrations[i] redone on the device with biases ba[i], bg[i] ([11][3])."""
        ba, bg = _f(ba).reshape(11, 3), _f(bg).reshape(11, 3)
        return self.L.lfvio_host_repropagate_window(self.h, _p(ba), _p(bg))

    # ---- SURVEY §8f rank 2
    def set_depths(self, depth):
        """estimated_depth of every feature in list order (the order load_window() added them)."""
        d = _f(depth)
        self.L.lfvio_host_set_depths(self.h, _p(d), len(d))

    def triangulate(self):
        return self.L.lfvio_host_triangulate(self.h)

    def remove_back_shift_depth(self, back_R0, back_P0):
        return self.L.lfvio_host_remove_back_shift_depth(self.h, _p(_f(back_R0)), _p(_f(back_P0)))

    def features(self):
        """(feature_id, start_frame, observation count, estimated_depth) arrays in list order."""
        n = self.L.lfvio_host_num_features(self.h)
        ids, st, cnt = (np.zeros(n, dtype=np.int32) for _ in range(3))
        dep = np.zeros(n)
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_list_features(self.h, ids.ctypes.data_as(ip), st.ctypes.data_as(ip), cnt.ctypes.data_as(ip), _p(dep))
        return ids, st, cnt, dep

    def pack(self):
        w = abi.WindowC()
        self.L.lfvio_host_pack(self.h, C.byref(w))
        return w

    def state(self):
        Ps, Rs, Vs, Bas, Bgs = np.zeros((11, 3)), np.zeros((11, 3, 3)), np.zeros((11, 3)), np.zeros((11, 3)), np.zeros((11, 3))
        tic, ric, td = np.zeros(3), np.zeros((3, 3)), np.zeros(1)
        self.L.lfvio_host_get_state(self.h, _p(Ps), _p(Rs), _p(Vs), _p(Bas), _p(Bgs), _p(tic), _p(ric), _p(td))
        return dict(Ps=Ps, Rs=Rs, Vs=Vs, Bas=Bas, Bgs=Bgs, tic=tic, ric=ric, td=float(td[0]))

    def para(self, n):
        pose, sb, ex, td, feat = np.zeros((11, 7)), np.zeros((11, 9)), np.zeros(7), np.zeros(1), np.zeros(max(n, 1))
        self.L.lfvio_host_get_para(self.h, _p(pose), _p(sb), _p(ex), _p(td), _p(feat))
        return pose, sb, ex, float(td[0]), feat[:n]

    def set_para(self, pose, sb, ex, td, feat):
        feat = _f(feat)
        self.L.lfvio_host_set_para(self.h, _p(_f(pose)), _p(_f(sb)), _p(_f(ex)), td, _p(feat), len(feat))

    def depths(self, n):
        d = np.zeros(max(n, 1))
        self.L.lfvio_host_get_depths(self.h, _p(d))
        return d[:n]

    # ---- relocalization (estimator.cpp:1133-1151, 603-625, 777-808)
    def set_relo_frame(self, stamp, index, match_points, relo_t, relo_r):
        """Estimator::setReloFrame: match_points [K, 3] = (x, y, id) sorted by id, relo_t [3], relo_r [3, 3]."""
        mp = _f(np.asarray(match_points, dtype=np.float64).reshape(-1, 3))
        self.L.lfvio_host_set_relo_frame.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp]
        self.L.lfvio_host_set_relo_frame(self.h, float(stamp), int(index), len(mp), _p(mp), _p(_f(relo_t)), _p(_f(relo_r)))

    def relo(self):
        """The relocalization members after optimization(): dict of relocalization_info, relo_frame_local_index, relo_Pose,
        drift_correct_r / t, relo_relative_t / q (x y z w) / yaw, relo_solves."""
        o = np.zeros(30)
        self.L.lfvio_host_get_relo.argtypes = [C.c_void_p, _dp]
        self.L.lfvio_host_get_relo(self.h, _p(o))
        return dict(relocalization_info=int(o[0]), relo_frame_local_index=int(o[1]), relo_Pose=o[2:9].copy(),
                    drift_correct_r=o[9:18].reshape(3, 3).copy(), drift_correct_t=o[18:21].copy(), relo_relative_t=o[21:24].copy(),
                    relo_relative_q=o[24:28].copy(), relo_relative_yaw=float(o[28]), relo_solves=int(o[29]))

    def relo_matches(self, cap=4096):
        """The match list of the reference's walk as optimization() would build it now -> (landmark[K], xy[K, 2])."""
        lm, xy = np.zeros(cap, dtype=np.int32), np.zeros((cap, 2))
        self.L.lfvio_host_relo_matches.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]
        K = self.L.lfvio_host_relo_matches(self.h, cap, lm.ctypes.data_as(C.POINTER(C.c_int)), _p(xy))
        return lm[:min(K, cap)].copy(), xy[:min(K, cap)].copy()

    # ---- ESTIMATE_EXTRINSIC == 2: the online camera-IMU rotation calibration (estimator.cpp:142-159, initial_ex_rotation.cpp)
    def set_params(self, p9, estimate_extrinsic, estimate_td, num_iterations):
        """The process-wide parameters: p9 = ACC_N, GYR_N, ACC_W, GYR_W, g, TR, ROW, SOLVER_TIME, TD."""
        self.L.lfvio_host_set_params(_p(_f(p9)), int(estimate_extrinsic), int(estimate_td), int(num_iterations))

    def set_extrinsic(self, tic, ric):
        """The CONFIGURED extrinsic (what a reset restores)."""
        self.L.lfvio_host_set_extrinsic.argtypes = [_dp, _dp]
        self.L.lfvio_host_set_extrinsic(_p(_f(tic)), _p(_f(ric).reshape(9)))

    def get_extrinsic(self):
        tic, ric = np.zeros(3), np.zeros(9)
        self.L.lfvio_host_get_extrinsic.argtypes = [_dp, _dp]
        self.L.lfvio_host_get_extrinsic(_p(tic), _p(ric))
        return tic, ric.reshape(3, 3)

    def estimate_extrinsic(self):
        return int(self.L.lfvio_host_get_estimate_extrinsic())

    def set_estimate_extrinsic(self, mode):
        self.L.lfvio_host_set_estimate_extrinsic.argtypes = [C.c_int]
        self.L.lfvio_host_set_estimate_extrinsic(int(mode))

    def exrot_last(self):
        """The pair the calibrator's last push added -> (Rc, Rimu)."""
        a, b = np.zeros(9), np.zeros(9)
        self.L.lfvio_host_exrot_last.argtypes = [C.c_void_p, _dp, _dp]
        self.L.lfvio_host_exrot_last(self.h, _p(a), _p(b))
        return a.reshape(3, 3), b.reshape(3, 3)

    def set_ransac(self, seed, iterations=100):
        self.L.lfvio_host_set_ransac.argtypes = [C.c_uint, C.c_int]
        self.L.lfvio_host_set_ransac(int(seed), int(iterations))

    def set_ric(self, ric):
        """The estimator's current ric alone (through lfvio_host_set_state, everything else as it is)."""
        s = self.state()
        self.L.lfvio_host_set_state(self.h, _p(_f(s["Ps"])), _p(_f(s["Rs"])), _p(_f(s["Vs"])), _p(_f(s["Bas"])), _p(_f(s["Bgs"])),
                                    _p(_f(s["tic"])), _p(_f(ric).reshape(9)), s["td"])

    def exrot_push(self, Rc, delta_q_xyzw):
        """CalibrationExRotation alone (no device) -> (success, ric [3, 3], singular values [4])."""
        ric, sv = np.zeros(9), np.zeros(4)
        self.L.lfvio_host_exrot_push.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        ok = self.L.lfvio_host_exrot_push(self.h, _p(_f(Rc).reshape(9)), _p(_f(delta_q_xyzw)), _p(ric), _p(sv))
        return bool(ok), ric.reshape(3, 3), sv

    def exrot_state(self):
        """-> (frame_count, ric, singular values) of the calibrator."""
        ric, sv = np.zeros(9), np.zeros(4)
        self.L.lfvio_host_exrot_state.argtypes = [C.c_void_p, _dp, _dp]
        n = self.L.lfvio_host_exrot_state(self.h, _p(ric), _p(sv))
        return int(n), ric.reshape(3, 3), sv

    def exrot_clear(self):
        self.L.lfvio_host_exrot_clear.argtypes = [C.c_void_p]
        self.L.lfvio_host_exrot_clear(self.h)

    def two_view_calls(self):
        self.L.lfvio_host_two_view_calls.argtypes = [C.c_void_p]
        self.L.lfvio_host_two_view_calls.restype = C.c_longlong
        return int(self.L.lfvio_host_two_view_calls(self.h))

    # ---- initialization from SfM poses
    def set_sfm(self, stamps, R, T):
        """An SfM result for the next full-window image: per frame its stamp, ImageFrame::R [n, 3, 3], ImageFrame::T [n, 3]."""
        st, R, T = _f(stamps).reshape(-1), _f(R).reshape(-1, 9), _f(T).reshape(-1, 3)
        self.L.lfvio_host_set_sfm.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        self.L.lfvio_host_set_sfm(self.h, len(st), _p(st), _p(R), _p(T))

    def set_sfm_structure(self, stamps, Q, T, ids, xyz):
        """What GlobalSFM::construct() returns, for the next full-window image: the window's keyframes (stamps [K], Q [K, 4] as
        w x y z, T [K, 3]: camera rotation and position in the SfM frame) and sfm_tracked_points (ids [P], xyz [P, 3]).  The
        estimator runs the PnP loop on it (lfvio_pnp) and then the alignment."""
        st, Q, T, xyz = _f(stamps).reshape(-1), _f(Q).reshape(-1, 4), _f(T).reshape(-1, 3), _f(xyz).reshape(-1, 3)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        assert len(st) == len(Q) == len(T) and len(ids) == len(xyz)
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_set_sfm_structure.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, ip, _dp]
        self.L.lfvio_host_set_sfm_structure.restype = None
        self.L.lfvio_host_set_sfm_structure(self.h, len(st), _p(st), _p(Q), _p(T), len(ids), ids.ctypes.data_as(ip), _p(xyz))

    def set_relative_pose(self, l, R, T):
        """What relativePose() returns, for the next full-window image: l, relative_R [3, 3], relative_T [3].  The estimator runs
        GlobalSFM::construct() on the device (lfvio_sfm_construct, lfvio_sfm_ba), then the PnP loop and the alignment."""
        R, T = _f(R).reshape(9), _f(T).reshape(3)
        self.L.lfvio_host_set_relative_pose.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        self.L.lfvio_host_set_relative_pose.restype = None
        self.L.lfvio_host_set_relative_pose(self.h, int(l), _p(R), _p(T))

    def sfm_structure(self, cap_kf=16, cap_pts=4096):
        """The SfM structure the estimator holds (what constructSfm() filled, or what was set): dict(stamps, Q [K, 4], T [K, 3], ids, xyz)."""
        cnt, ids = np.zeros(2, dtype=np.int32), np.zeros(cap_pts, dtype=np.int32)
        st, Q, T, xyz = np.zeros(cap_kf), np.zeros((cap_kf, 4)), np.zeros((cap_kf, 3)), np.zeros((cap_pts, 3))
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_get_sfm_structure.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, _dp, _dp, _dp, ip, _dp]
        self.L.lfvio_host_get_sfm_structure.restype = None
        self.L.lfvio_host_get_sfm_structure(self.h, cap_kf, cap_pts, cnt.ctypes.data_as(ip), _p(st), _p(Q), _p(T), ids.ctypes.data_as(ip), _p(xyz))
        K, P = min(int(cnt[0]), cap_kf), min(int(cnt[1]), cap_pts)
        return dict(stamps=st[:K].copy(), Q=Q[:K].copy(), T=T[:K].copy(), ids=ids[:P].copy(), xyz=xyz[:P].copy())

    def last_construct(self, cap_points=4096, cap_obs=4096 * 11):
        """What the last attempt passed to lfvio_sfm_construct / lfvio_sfm_ba and got back: dict(F, l, ids, offset, frame, bearing,
        relative_R, relative_T, c_rotation, c_translation, position, tri_op (as lfvio_sfm_construct left them), out (the fields of
        LfvioSfmConstructOut), ba (those of LfvioSfmBaOut), called, rc, ba_called, ba_rc, calls)."""
        info = np.zeros(8, dtype=np.int32)
        ids, off, frm, ops = (np.zeros(n, dtype=np.int32) for n in (cap_points, cap_points + 1, cap_obs, cap_points))
        us, rel, q, t, X = np.zeros((cap_obs, 3)), np.zeros(12), np.zeros((abi.NUM_FRAMES, 4)), np.zeros((abi.NUM_FRAMES, 3)), np.zeros((cap_points, 3))
        out, ba = abi.SfmConstructOutC(), abi.SfmBaOutC()
        ip = C.POINTER(C.c_int)
        i_ = lambda a: a.ctypes.data_as(ip)
        self.L.lfvio_host_last_construct.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, ip, ip, _dp, _dp, _dp, _dp, _dp, ip,
                                                     C.POINTER(abi.SfmConstructOutC), C.POINTER(abi.SfmBaOutC)]
        self.L.lfvio_host_last_construct.restype = C.c_longlong
        calls = self.L.lfvio_host_last_construct(self.h, cap_points, cap_obs, i_(info), i_(ids), i_(off), i_(frm), _p(us), _p(rel), _p(q), _p(t), _p(X), i_(ops),
                                                 C.byref(out), C.byref(ba))
        F, l, P, M = (int(v) for v in info[:4])
        return dict(F=F, l=l, ids=ids[:P].copy(), offset=off[:P + 1].copy(), frame=frm[:M].copy(), bearing=us[:M].copy(), relative_R=rel[:9].reshape(3, 3).copy(),
                    relative_T=rel[9:].copy(), c_rotation=q[:F].copy(), c_translation=t[:F].copy(), position=X[:P].copy(), tri_op=ops[:P].copy(),
                    out=out.as_dict(min(F, abi.NUM_FRAMES)) if info[4] else None, ba=ba.as_dict(min(F, abi.NUM_FRAMES)) if info[6] else None,
                    called=bool(info[4]), rc=int(info[5]), ba_called=bool(info[6]), ba_rc=int(info[7]), calls=int(calls))

    def construct_counts(self):
        """(attempts that reached lfvio_sfm_construct, attempts that filled the SfM structure)."""
        o = np.zeros(2, dtype=np.int64)
        self.L.lfvio_host_construct_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self.L.lfvio_host_construct_counts(self.h, o.ctypes.data_as(C.POINTER(C.c_longlong)))
        return int(o[0]), int(o[1])

    def set_self_relative_pose(self, on):
        """Config::self_relative_pose (process-wide): a full-window image for which no record of any kind was set runs relativePose()
        on the device (lfvio_relative_pose) and initializes from its own measurements."""
        self.L.lfvio_host_set_self_relative_pose.argtypes = [C.c_int]
        self.L.lfvio_host_set_self_relative_pose.restype = None
        self.L.lfvio_host_set_self_relative_pose(int(bool(on)))

    def last_relative(self):
        """What the last attempt passed to lfvio_relative_pose and got back: dict(offset [P + 1], bl, br [M, 3], samples [P, S, 8], out
        (the fields of LfvioRelativePoseOut, None without a device call), called, rc, calls)."""
        P = abi.WINDOW_SIZE
        info, off = np.zeros(4, dtype=np.int32), np.zeros(P + 1, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        i_ = lambda a: a.ctypes.data_as(ip)
        self.L.lfvio_host_last_relative.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, _dp, _dp, ip, C.POINTER(abi.RelativePoseOutC)]
        self.L.lfvio_host_last_relative.restype = C.c_longlong
        self.L.lfvio_host_last_relative(self.h, 0, 0, i_(info), i_(off), None, None, None, None)  # the sizes first
        M, S = int(info[0]), int(info[1])
        bl, br, sm, out = np.zeros((max(M, 1), 3)), np.zeros((max(M, 1), 3)), np.zeros((P, max(S, 1), 8), dtype=np.int32), abi.RelativePoseOutC()
        calls = self.L.lfvio_host_last_relative(self.h, max(M, 1), max(S, 1), i_(info), i_(off), _p(bl), _p(br), i_(sm), C.byref(out))
        return dict(offset=off, bl=bl[:M].copy(), br=br[:M].copy(), samples=sm[:, :S].copy(), out=out.as_dict() if info[2] else None,
                    called=bool(info[2]), rc=int(info[3]), calls=int(calls))

    def relative_counts(self):
        """(attempts that reached lfvio_relative_pose, attempts that filled the relative pose)."""
        o = np.zeros(2, dtype=np.int64)
        self.L.lfvio_host_relative_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self.L.lfvio_host_relative_counts(self.h, o.ctypes.data_as(C.POINTER(C.c_longlong)))
        return int(o[0]), int(o[1])

    def draw_pair_samples(self, seed, counts, num_sets):
        """The sample sets relativePose() draws from std::mt19937(seed) for pairs of counts[p] matches: num_sets per pair with more than
        20 matches, pair order, then set order -> [P, num_sets, 8] (zeros for the other pairs)."""
        n = np.ascontiguousarray(counts, dtype=np.int32)
        o = np.zeros((len(n), num_sets, 8), dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_draw_pair_samples.argtypes = [C.c_uint, C.c_int, ip, C.c_int, ip]
        self.L.lfvio_host_draw_pair_samples.restype = None
        self.L.lfvio_host_draw_pair_samples(int(seed), len(n), n.ctypes.data_as(ip), int(num_sets), o.ctypes.data_as(ip))
        return o

    def sfm(self, cap=1024):
        """The SfM result the estimator holds (after the PnP loop: every frame of all_image_frame): (stamps, R [n, 3, 3], T [n, 3])."""
        st, R, T = np.zeros(cap), np.zeros((cap, 9)), np.zeros((cap, 3))
        self.L.lfvio_host_get_sfm.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        n = min(self.L.lfvio_host_get_sfm(self.h, cap, _p(st), _p(R), _p(T)), cap)
        return st[:n].copy(), R[:n].reshape(n, 3, 3).copy(), T[:n].copy()

    def image_frame_points(self, k, cap=4096):
        """ImageFrame::points of entry k of all_image_frame: (ids ascending, bearings [n, 3]); None when there is no such entry."""
        ids, pts = np.zeros(cap, dtype=np.int32), np.zeros((cap, 3))
        self.L.lfvio_host_image_frame_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), _dp]
        n = self.L.lfvio_host_image_frame_points(self.h, int(k), cap, ids.ctypes.data_as(C.POINTER(C.c_int)), _p(pts))
        return None if n < 0 else (ids[:n].copy(), pts[:n].copy())

    def last_pnp(self, cap_frames=128, cap_points=1 << 17):
        """What the last attempt passed to lfvio_pnp and got back: dict(stamps (of the non-keyframes), offset, pw, us, out (a list of
        the fields of LfvioPnpOut), called, rc, calls)."""
        info = np.zeros(4, dtype=np.int32)
        st, off = np.zeros(cap_frames), np.zeros(cap_frames + 1, dtype=np.int32)
        pw, us, out = np.zeros((cap_points, 3)), np.zeros((cap_points, 3)), (abi.PnpOutC * cap_frames)()
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_last_pnp.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, _dp, ip, _dp, _dp, C.POINTER(abi.PnpOutC)]
        self.L.lfvio_host_last_pnp.restype = C.c_longlong
        calls = self.L.lfvio_host_last_pnp(self.h, cap_frames, cap_points, info.ctypes.data_as(ip), _p(st), off.ctypes.data_as(ip), _p(pw), _p(us), out)
        F, M = int(info[0]), int(info[1])
        return dict(stamps=st[:F].copy(), offset=off[:F + 1].copy(), pw=pw[:M].copy(), us=us[:M].copy(),
                    out=[out[f].as_dict() for f in range(F)] if info[2] else [], called=bool(info[2]), rc=int(info[3]), calls=int(calls))

    def set_td(self, td):
        """The CONFIGURED time offset (what a reset restores); with set_extrinsic() what a recording without bootstrap records needs."""
        self.L.lfvio_host_set_td.argtypes = [C.c_double]
        self.L.lfvio_host_set_td(float(td))

    def set_stop_after_align(self, on):
        """Tests: process_image() returns right behind a successful visualInitialAlign(), the window as the alignment left it."""
        self.L.lfvio_host_set_stop_after_align.argtypes = [C.c_void_p, C.c_int]
        self.L.lfvio_host_set_stop_after_align(self.h, int(on))

    def gravity(self):
        g = np.zeros(3)
        self.L.lfvio_host_get_gravity.argtypes = [C.c_void_p, _dp]
        self.L.lfvio_host_get_gravity(self.h, _p(g))
        return g

    def image_frames(self, cap=1024):
        """all_image_frame: (stamps, samples per entry)."""
        st, ns = np.zeros(cap), np.zeros(cap, dtype=np.int32)
        self.L.lfvio_host_image_frames.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int)]
        n = self.L.lfvio_host_image_frames(self.h, cap, _p(st), ns.ctypes.data_as(C.POINTER(C.c_int)))
        return st[:n].copy(), ns[:n].copy()

    def vi_align_counts(self):
        """(attempts that reached lfvio_vi_align, attempts that aligned)."""
        o = np.zeros(2, dtype=np.int64)
        self.L.lfvio_host_vi_align_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self.L.lfvio_host_vi_align_counts(self.h, o.ctypes.data_as(C.POINTER(C.c_longlong)))
        return int(o[0]), int(o[1])

    def last_vi_align(self, cap_frames=128, cap_samples=1 << 16):
        """What the last attempt passed to lfvio_vi_align and got back: dict(R, T, stamps, spans (the tuples Engine.vi_align
        takes, entry 0 None), noise, tic, G, out (the fields of LfvioViAlignOut), x, called, rc, calls)."""
        info = np.zeros(4, dtype=np.int32)
        st, R, T = np.zeros(cap_frames), np.zeros((cap_frames, 9)), np.zeros((cap_frames, 3))
        cnt, head = np.zeros(cap_frames, dtype=np.int32), np.zeros((cap_frames, 12))
        dt, acc, gyr = np.zeros(cap_samples), np.zeros((cap_samples, 3)), np.zeros((cap_samples, 3))
        prm, x, out = np.zeros(8), np.zeros(3 * cap_frames), abi.ViAlignOutC()
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_last_vi_align.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, _dp, _dp, _dp, ip, _dp, _dp, _dp, _dp, _dp, C.POINTER(abi.ViAlignOutC), _dp]
        self.L.lfvio_host_last_vi_align.restype = C.c_longlong
        calls = self.L.lfvio_host_last_vi_align(self.h, cap_frames, cap_samples, info.ctypes.data_as(ip), _p(st), _p(R), _p(T), cnt.ctypes.data_as(ip),
                                                _p(head), _p(dt), _p(acc), _p(gyr), _p(prm), C.byref(out), _p(x))
        F = int(info[0])
        spans, o = [None], 0
        for k in range(1, F):
            n = int(cnt[k])
            spans.append((head[k, 0:3].copy(), head[k, 3:6].copy(), head[k, 6:9].copy(), head[k, 9:12].copy(), dt[o:o + n].copy(), acc[o:o + n].copy(), gyr[o:o + n].copy()))
            o += n
        return dict(stamps=st[:F].copy(), R=R[:F].reshape(F, 3, 3).copy(), T=T[:F].copy(), spans=spans, noise=prm[0:4].copy(), tic=prm[4:7].copy(),
                    G=float(prm[7]), out=out.as_dict(), x=x[:3 * F].copy(), called=bool(info[2]), rc=int(info[3]), calls=int(calls))

    def last_two_view(self, cap_matches=4096, cap_samples=1024):
        """What the last image of mode 2 handed to lfvio_two_view and got back: dict(bl, br, samples, mask, out (the fields of
        LfvioTwoViewOut, None without a device call), calls)."""
        cnt = np.zeros(2, dtype=np.int32)
        bl, br = np.zeros((cap_matches, 3)), np.zeros((cap_matches, 3))
        sm, mask, out = np.zeros((cap_samples, 8), dtype=np.int32), np.zeros(cap_matches, dtype=np.uint8), abi.TwoViewOutC()
        ip = C.POINTER(C.c_int)
        self.L.lfvio_host_last_two_view.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, _dp, _dp, ip, C.POINTER(C.c_ubyte), C.POINTER(abi.TwoViewOutC)]
        self.L.lfvio_host_last_two_view.restype = C.c_longlong
        calls = self.L.lfvio_host_last_two_view(self.h, cap_matches, cap_samples, cnt.ctypes.data_as(ip), _p(bl), _p(br), sm.ctypes.data_as(ip),
                                                mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out))
        N, S = int(cnt[0]), int(cnt[1])
        return dict(bl=bl[:N].copy(), br=br[:N].copy(), samples=sm[:S].copy(), mask=mask[:N].copy(), out=out.as_dict() if S else None, calls=int(calls))

    def corresponding(self, l, r, cap=4096):
        """FeatureManager::getCorresponding(l, r) -> (bl [n, 3], br [n, 3])."""
        bl, br = np.zeros((cap, 3)), np.zeros((cap, 3))
        self.L.lfvio_host_corresponding.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp]
        n = self.L.lfvio_host_corresponding(self.h, int(l), int(r), cap, _p(bl), _p(br))
        return bl[:n].copy(), br[:n].copy()

    def draw_samples(self, seed, n, count):
        """util::create_random_array(8, 0, n - 1), `count` times from std::mt19937(seed) -> [count, 8]."""
        o = np.zeros((count, 8), dtype=np.int32)
        self.L.lfvio_host_draw_samples.argtypes = [C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int)]
        self.L.lfvio_host_draw_samples(int(seed), int(n), int(count), o.ctypes.data_as(C.POINTER(C.c_int)))
        return o

    def set_split_call(self, on):
        self.L.lfvio_host_set_split_call(int(on))

    def set_device_chain(self, on):
        self.L.lfvio_host_set_device_chain.argtypes = [C.c_int]
        self.L.lfvio_host_set_device_chain(int(on))

    def optimization(self, flag, fused=True):
        self.L.lfvio_host_set_flag(self.h, flag)
        self.L.lfvio_host_set_fused(self.h, int(fused))
        return self.L.lfvio_host_optimization(self.h)

    def prior(self):
        p = abi.Prior()
        self.L.lfvio_host_get_prior(self.h, C.byref(p))
        return p
