"""ctypes mirror of include/lfvio.h (the C-ABI boundary).

The structs here are laid out exactly like the C PODs; `Window` keeps the numpy
arrays that back the pointer members alive.  Nothing in this module computes
anything: it is plumbing between Python (tests / bench) and the C-ABI library.
"""
import ctypes as C
import os

import numpy as np

WINDOW_SIZE = 10
NUM_FRAMES = 11
MAX_PRIOR_BLOCKS = 24
MAX_PRIOR_DIM = 172
MAX_TRACE = 64
SIZE_POSE = 7

OK = 0
MARGIN_OLD = 0
MAIL_MAX_LM = 8192  # csrc/dev_types.h: largest window whose solution lfvio_batch_optimize_begin hands over early
MARGIN_SECOND_NEW = 1
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
BLOCK_POSE, BLOCK_SPEEDBIAS, BLOCK_EX_POSE, BLOCK_TD = 0, 1, 2, 3

# tangent layout shared by the oracle, the HIP path and the tests (P = 172):
KC, KP = 73, 172


def off_pose(f):
    return 6 * f


OFF_EX, OFF_TD = 66, 72


def off_sb(f):
    return 73 + 9 * f


c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)


class BlockId(C.Structure):
    _fields_ = [("kind", C.c_int), ("frame", C.c_int)]


class Preintegration(C.Structure):
    _fields_ = [
        ("sum_dt", C.c_double),
        ("delta_p", C.c_double * 3),
        ("delta_q", C.c_double * 4),
        ("delta_v", C.c_double * 3),
        ("linearized_ba", C.c_double * 3),
        ("linearized_bg", C.c_double * 3),
        ("jacobian", C.c_double * 225),
        ("covariance", C.c_double * 225),
    ]


class ImuIntervalC(C.Structure):
    _fields_ = [
        ("num_samples", C.c_int),
        ("dt", C.POINTER(C.c_double)),
        ("acc", C.POINTER(C.c_double)),
        ("gyr", C.POINTER(C.c_double)),
        ("acc_0", C.c_double * 3),
        ("gyr_0", C.c_double * 3),
        ("linearized_ba", C.c_double * 3),
        ("linearized_bg", C.c_double * 3),
    ]


class Prior(C.Structure):
    _fields_ = [
        ("valid", C.c_int),
        ("m", C.c_int),
        ("n", C.c_int),
        ("num_blocks", C.c_int),
        ("blocks", BlockId * MAX_PRIOR_BLOCKS),
        ("block_idx", C.c_int * MAX_PRIOR_BLOCKS),
        ("block_x0", (C.c_double * 9) * MAX_PRIOR_BLOCKS),
        ("linearized_jacobians", C.c_double * (MAX_PRIOR_DIM * MAX_PRIOR_DIM)),
        ("linearized_residuals", C.c_double * MAX_PRIOR_DIM),
    ]

    def J(self):
        n = self.n
        return np.frombuffer(self.linearized_jacobians, dtype=np.float64, count=n * n).reshape(n, n).copy()

    def r(self):
        return np.frombuffer(self.linearized_residuals, dtype=np.float64, count=self.n).copy()

    def block_list(self):
        return [(self.blocks[i].kind, self.blocks[i].frame, self.block_idx[i]) for i in range(self.num_blocks)]

    def x0(self, i):
        return np.array(self.block_x0[i][:], dtype=np.float64)


class WindowC(C.Structure):
    _fields_ = [
        ("para_pose", (C.c_double * 7) * NUM_FRAMES),
        ("para_speed_bias", (C.c_double * 9) * NUM_FRAMES),
        ("para_ex_pose", C.c_double * 7),
        ("para_td", C.c_double),
        ("estimate_extrinsic", C.c_int),
        ("estimate_td", C.c_int),
        ("max_num_iterations", C.c_int),
        ("max_solver_time_in_seconds", C.c_double),
        ("g", C.c_double * 3),
        ("tr", C.c_double),
        ("row", C.c_double),
        ("sqrt_info", C.c_double),
        ("num_landmarks", C.c_int),
        ("num_observations", C.c_int),
        ("start_frame", c_int_p),
        ("obs_offset", c_int_p),
        ("inv_depth", c_double_p),
        ("obs_point", c_double_p),
        ("obs_velocity", c_double_p),
        ("obs_cur_td", c_double_p),
        ("obs_uv_y", c_double_p),
        ("imu", Preintegration * WINDOW_SIZE),
        ("prior", C.POINTER(Prior)),
    ]


class IterationSummary(C.Structure):
    _fields_ = [
        ("cost", C.c_double),
        ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("step_norm", C.c_double),
        ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double),
        ("step_is_valid", C.c_int),
        ("step_is_successful", C.c_int),
    ]


class SolutionC(C.Structure):
    _fields_ = [
        ("para_pose", (C.c_double * 7) * NUM_FRAMES),
        ("para_speed_bias", (C.c_double * 9) * NUM_FRAMES),
        ("para_ex_pose", C.c_double * 7),
        ("para_td", C.c_double),
        ("inv_depth", c_double_p),
        ("num_iterations", C.c_int),
        ("num_successful_steps", C.c_int),
        ("num_unsuccessful_steps", C.c_int),
        ("termination", C.c_int),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("trace", IterationSummary * MAX_TRACE),
    ]


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class Window:
    """Python-side owner of one LfvioWindow (numpy arrays + the C struct)."""

    def __init__(self, pose, speed_bias, ex_pose, td, start_frame, obs_offset, inv_depth, obs_point, obs_velocity,
                 obs_cur_td, obs_uv_y, imu, prior=None, estimate_extrinsic=1, estimate_td=1, max_num_iterations=8,
                 max_solver_time=-1.0, g=(0.0, 0.0, 9.81007), tr=0.0, row=960.0, sqrt_info=160.0 / 1.5):
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.pose = f64(pose).reshape(NUM_FRAMES, 7)
        self.speed_bias = f64(speed_bias).reshape(NUM_FRAMES, 9)
        self.ex_pose = f64(ex_pose).reshape(7)
        self.td = float(td)
        self.start_frame = np.ascontiguousarray(start_frame, dtype=np.int32)
        self.obs_offset = np.ascontiguousarray(obs_offset, dtype=np.int32)
        self.inv_depth = f64(inv_depth)
        self.obs_point = f64(obs_point).reshape(-1, 3)
        self.obs_velocity = f64(obs_velocity).reshape(-1, 3)
        self.obs_cur_td = f64(obs_cur_td)
        self.obs_uv_y = f64(obs_uv_y)
        self.imu = imu  # list of 10 Preintegration
        self.prior = prior  # Prior or None
        self.estimate_extrinsic = int(estimate_extrinsic)
        self.estimate_td = int(estimate_td)
        self.max_num_iterations = int(max_num_iterations)
        self.max_solver_time = float(max_solver_time)
        self.g = tuple(float(v) for v in g)
        self.tr, self.row, self.sqrt_info = float(tr), float(row), float(sqrt_info)
        self._c = None

    @property
    def N(self):
        return int(self.start_frame.shape[0])

    @property
    def M(self):
        return int(self.obs_point.shape[0])

    def copy(self, **over):
        kw = dict(pose=self.pose.copy(), speed_bias=self.speed_bias.copy(), ex_pose=self.ex_pose.copy(), td=self.td,
                  start_frame=self.start_frame.copy(), obs_offset=self.obs_offset.copy(),
                  inv_depth=self.inv_depth.copy(), obs_point=self.obs_point.copy(),
                  obs_velocity=self.obs_velocity.copy(), obs_cur_td=self.obs_cur_td.copy(),
                  obs_uv_y=self.obs_uv_y.copy(), imu=self.imu, prior=self.prior,
                  estimate_extrinsic=self.estimate_extrinsic, estimate_td=self.estimate_td,
                  max_num_iterations=self.max_num_iterations, max_solver_time=self.max_solver_time, g=self.g,
                  tr=self.tr, row=self.row, sqrt_info=self.sqrt_info)
        kw.update(over)
        return Window(**kw)

    def c(self):
        """(Re)build the C struct; call after mutating any field."""
        w = WindowC()
        for f in range(NUM_FRAMES):
            for k in range(7):
                w.para_pose[f][k] = self.pose[f, k]
            for k in range(9):
                w.para_speed_bias[f][k] = self.speed_bias[f, k]
        for k in range(7):
            w.para_ex_pose[k] = self.ex_pose[k]
        w.para_td = self.td
        w.estimate_extrinsic = self.estimate_extrinsic
        w.estimate_td = self.estimate_td
        w.max_num_iterations = self.max_num_iterations
        w.max_solver_time_in_seconds = self.max_solver_time
        for k in range(3):
            w.g[k] = self.g[k]
        w.tr, w.row, w.sqrt_info = self.tr, self.row, self.sqrt_info
        w.num_landmarks = self.N
        w.num_observations = self.M
        assert self.obs_offset.shape[0] == self.N + 1 and int(self.obs_offset[-1]) == self.M
        w.start_frame = _ptr(self.start_frame, C.c_int)
        w.obs_offset = _ptr(self.obs_offset, C.c_int)
        w.inv_depth = _ptr(self.inv_depth, C.c_double)
        w.obs_point = _ptr(self.obs_point, C.c_double)
        w.obs_velocity = _ptr(self.obs_velocity, C.c_double)
        w.obs_cur_td = _ptr(self.obs_cur_td, C.c_double)
        w.obs_uv_y = _ptr(self.obs_uv_y, C.c_double)
        for i in range(WINDOW_SIZE):
            w.imu[i] = self.imu[i]
        w.prior = C.pointer(self.prior) if (self.prior is not None and self.prior.valid) else None
        self._c = w
        return w


class ReloC(C.Structure):
    """LfvioRelo (include/lfvio.h): one relocalization message as the solve consumes it."""
    _fields_ = [("frame", C.c_int), ("relo_pose", C.c_double * SIZE_POSE), ("num_matches", C.c_int),
                ("landmark", C.POINTER(C.c_int)), ("match_point", C.POINTER(C.c_double))]


class Relo:
    """Owns the arrays behind a ReloC: frame, initial relo pose [p, q xyzw], landmark indices [K], match points [K][2]."""

    def __init__(self, frame, relo_pose, landmark=(), match_point=()):
        self.frame = int(frame)
        self.relo_pose = np.ascontiguousarray(relo_pose, dtype=np.float64).reshape(SIZE_POSE)
        self.landmark = np.ascontiguousarray(landmark, dtype=np.int32).reshape(-1)
        self.match_point = np.ascontiguousarray(match_point, dtype=np.float64).reshape(-1, 2)
        self._c = None

    @property
    def K(self):
        return int(self.landmark.size)

    def c(self, num_matches=None, null_arrays=False):
        r = ReloC()
        r.frame = self.frame
        for k in range(SIZE_POSE):
            r.relo_pose[k] = float(self.relo_pose[k])
        r.num_matches = self.K if num_matches is None else int(num_matches)
        if not null_arrays and self.K > 0:
            r.landmark = _ptr(self.landmark, C.c_int)
            r.match_point = _ptr(self.match_point, C.c_double)
        self._c = r
        return r


class Solution:
    def __init__(self, n_landmarks):
        self.inv_depth = np.zeros(max(n_landmarks, 1), dtype=np.float64)
        self.c = SolutionC()
        self.c.inv_depth = _ptr(self.inv_depth, C.c_double)
        self.N = n_landmarks

    @property
    def pose(self):
        return np.array([[self.c.para_pose[f][k] for k in range(7)] for f in range(NUM_FRAMES)])

    @property
    def speed_bias(self):
        return np.array([[self.c.para_speed_bias[f][k] for k in range(9)] for f in range(NUM_FRAMES)])

    @property
    def ex_pose(self):
        return np.array(self.c.para_ex_pose[:])

    @property
    def td(self):
        return float(self.c.para_td)

    @property
    def lam(self):
        return self.inv_depth[: self.N].copy()

    def trace(self):
        out = []
        for k in range(min(self.c.num_iterations, MAX_TRACE)):
            t = self.c.trace[k]
            out.append(dict(cost=t.cost, cost_change=t.cost_change, gradient_max_norm=t.gradient_max_norm,
                            step_norm=t.step_norm, relative_decrease=t.relative_decrease,
                            radius=t.trust_region_radius, valid=t.step_is_valid, successful=t.step_is_successful))
        return out


def apply_solution(win, sol):
    """Window whose state is the solution's (used between solve and marginalize)."""
    return win.copy(pose=sol.pose, speed_bias=sol.speed_bias, ex_pose=sol.ex_pose, td=sol.td, inv_depth=sol.lam)


PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_LIB_PATH = os.path.join(PKG_DIR, "liblfvio_hip.so")

class TriangulateInC(C.Structure):
    """LfvioTriangulateIn (include/lfvio.h)."""
    _fields_ = [
        ("num_landmarks", C.c_int),
        ("num_observations", C.c_int),
        ("start_frame", C.POINTER(C.c_int)),
        ("obs_offset", C.POINTER(C.c_int)),
        ("obs_point", C.POINTER(C.c_double)),
        ("Ps", (C.c_double * 3) * NUM_FRAMES),
        ("Rs", (C.c_double * 9) * NUM_FRAMES),
        ("tic", C.c_double * 3),
        ("ric", C.c_double * 9),
        ("init_depth", C.c_double),
    ]


class TriangulateIn:
    """Inputs of FeatureManager::triangulate taken from a window: frame poses (Ps, Rs), extrinsics, the landmark CSR and
    the stored observation points.  Keeps the numpy arrays alive for the ctypes view."""

    def __init__(self, win, Rs=None, ric=None, init_depth=5.0):
        from . import synth  # quaternion helpers

        self.start_frame = np.ascontiguousarray(win.start_frame, dtype=np.int32)
        self.obs_offset = np.ascontiguousarray(win.obs_offset, dtype=np.int32)
        self.obs_point = np.ascontiguousarray(win.obs_point, dtype=np.float64).reshape(-1, 3)
        self.Ps = np.ascontiguousarray(win.pose[:, :3], dtype=np.float64)
        self.Rs = np.stack([synth.pose_R(win.pose[f]) for f in range(NUM_FRAMES)]) if Rs is None else np.asarray(Rs, float)
        self.tic = np.ascontiguousarray(win.ex_pose[:3], dtype=np.float64)
        self.ric = synth.pose_R(win.ex_pose) if ric is None else np.asarray(ric, float)
        self.init_depth = float(init_depth)
        c = TriangulateInC()
        c.num_landmarks, c.num_observations = len(self.start_frame), len(self.obs_point)
        c.start_frame = self.start_frame.ctypes.data_as(C.POINTER(C.c_int))
        c.obs_offset = self.obs_offset.ctypes.data_as(C.POINTER(C.c_int))
        c.obs_point = self.obs_point.ctypes.data_as(C.POINTER(C.c_double))
        for f in range(NUM_FRAMES):
            for k in range(3):
                c.Ps[f][k] = self.Ps[f, k]
            for k in range(9):
                c.Rs[f][k] = self.Rs[f].reshape(9)[k]
        for k in range(3):
            c.tic[k] = self.tic[k]
        for k in range(9):
            c.ric[k] = self.ric.reshape(9)[k]
        c.init_depth = self.init_depth
        self.c = c


class TwoViewInC(C.Structure):
    """LfvioTwoViewIn (include/lfvio.h)."""
    _fields_ = [
        ("num_matches", C.c_int),
        ("bearing_l", C.POINTER(C.c_double)),
        ("bearing_r", C.POINTER(C.c_double)),
        ("num_samples", C.c_int),
        ("samples", C.POINTER(C.c_int)),
    ]


class TwoViewOutC(C.Structure):
    """LfvioTwoViewOut (include/lfvio.h)."""
    _fields_ = [
        ("status", C.c_int),
        ("best_sample", C.c_int),
        ("num_inliers", C.c_int),
        ("best_score", C.c_double),
        ("E", C.c_double * 9),
        ("R_cand", (C.c_double * 9) * 2),
        ("t_cand", C.c_double * 3),
        ("front", C.c_double * 4),
        ("R_rel", C.c_double * 9),
    ]

    def as_dict(self):
        a = lambda x: np.array(x, dtype=np.float64)
        return dict(status=int(self.status), best_sample=int(self.best_sample), num_inliers=int(self.num_inliers),
                    best_score=float(self.best_score), E=a(self.E), R_cand=np.array([list(self.R_cand[0]), list(self.R_cand[1])]).reshape(2, 3, 3),
                    t_cand=a(self.t_cand), front=a(self.front), R_rel=a(self.R_rel).reshape(3, 3))


MAX_IMAGE_FRAMES = 128  # LFVIO_MAX_IMAGE_FRAMES


class ViAlignInC(C.Structure):
    """LfvioViAlignIn (include/lfvio.h)."""
    _fields_ = [
        ("num_frames", C.c_int),
        ("R", C.POINTER(C.c_double)),
        ("T", C.POINTER(C.c_double)),
        ("span", C.POINTER(ImuIntervalC)),
        ("noise", C.c_double * 4),
        ("tic", C.c_double * 3),
        ("g_norm", C.c_double),
    ]


class ViAlignOutC(C.Structure):
    """LfvioViAlignOut (include/lfvio.h)."""
    _fields_ = [
        ("status", C.c_int),
        ("delta_bg", C.c_double * 3),
        ("g_linear", C.c_double * 3),
        ("s_linear", C.c_double),
        ("g_iter", (C.c_double * 3) * 4),
        ("g", C.c_double * 3),
        ("s", C.c_double),
    ]

    def as_dict(self):
        a = lambda x: np.array(x, dtype=np.float64)
        return dict(status=int(self.status), delta_bg=a(self.delta_bg), g_linear=a(self.g_linear), s_linear=float(self.s_linear),
                    g_iter=np.array([list(r) for r in self.g_iter], dtype=np.float64), g=a(self.g), s=float(self.s))


class PnpInC(C.Structure):
    """LfvioPnpIn (include/lfvio.h)."""
    _fields_ = [
        ("num_frames", C.c_int),
        ("offset", C.POINTER(C.c_int)),
        ("point_w", C.POINTER(C.c_double)),
        ("bearing", C.POINTER(C.c_double)),
    ]


class PnpOutC(C.Structure):
    """LfvioPnpOut (include/lfvio.h)."""
    _fields_ = [
        ("status", C.c_int),
        ("chosen", C.c_int),
        ("R", C.c_double * 9),
        ("T", C.c_double * 3),
        ("err", C.c_double * 3),
    ]

    def as_dict(self):
        a = lambda x: np.array(x, dtype=np.float64)
        return dict(status=int(self.status), chosen=int(self.chosen), R=a(self.R).reshape(3, 3), T=a(self.T), err=a(self.err))


PNP_MIN_POINTS, PNP_MAX_POINTS = 6, 4096


class SfmBaInC(C.Structure):
    """LfvioSfmBaIn (include/lfvio.h)."""
    _fields_ = [
        ("num_frames", C.c_int),
        ("ref_frame", C.c_int),
        ("num_points", C.c_int),
        ("obs_offset", C.POINTER(C.c_int)),
        ("obs_frame", C.POINTER(C.c_int)),
        ("obs_bearing", C.POINTER(C.c_double)),
        ("max_num_iterations", C.c_int),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
    ]


class SfmBaOutC(C.Structure):
    """LfvioSfmBaOut (include/lfvio.h)."""
    _fields_ = [
        ("termination", C.c_int),
        ("num_iterations", C.c_int),
        ("num_successful_steps", C.c_int),
        ("num_unsuccessful_steps", C.c_int),
        ("accepted", C.c_int),
        ("pad_", C.c_int),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("Q", (C.c_double * 4) * NUM_FRAMES),
        ("T", (C.c_double * 3) * NUM_FRAMES),
        ("trace", IterationSummary * MAX_TRACE),
    ]

    def as_dict(self, F=NUM_FRAMES):
        n = min(int(self.num_iterations), MAX_TRACE)
        trace = [{k: getattr(self.trace[i], k) for k, _ in IterationSummary._fields_} for i in range(max(n, 0))]
        return dict(termination=int(self.termination), num_iterations=int(self.num_iterations), num_successful_steps=int(self.num_successful_steps),
                    num_unsuccessful_steps=int(self.num_unsuccessful_steps), accepted=int(self.accepted), initial_cost=float(self.initial_cost),
                    final_cost=float(self.final_cost), Q=np.array([list(r) for r in self.Q], dtype=np.float64)[:F],
                    T=np.array([list(r) for r in self.T], dtype=np.float64)[:F], trace=trace)


SFMBA_MAX_POINTS = 4096


class SfmConstructInC(C.Structure):
    """LfvioSfmConstructIn (include/lfvio.h)."""
    _fields_ = [
        ("num_frames", C.c_int),
        ("ref_frame", C.c_int),
        ("num_points", C.c_int),
        ("obs_offset", C.POINTER(C.c_int)),
        ("obs_frame", C.POINTER(C.c_int)),
        ("obs_bearing", C.POINTER(C.c_double)),
        ("relative_R", C.c_double * 9),
        ("relative_T", C.c_double * 3),
    ]


class SfmConstructOutC(C.Structure):
    """LfvioSfmConstructOut (include/lfvio.h)."""
    _fields_ = [
        ("status", C.c_int),
        ("failed_frame", C.c_int),
        ("num_triangulated", C.c_int),
        ("pad_", C.c_int),
        ("pnp_op", C.c_int * NUM_FRAMES),
        ("pnp_count", C.c_int * NUM_FRAMES),
        ("pnp", PnpOutC * NUM_FRAMES),
    ]

    def as_dict(self, F=NUM_FRAMES):
        return dict(status=int(self.status), failed_frame=int(self.failed_frame), num_triangulated=int(self.num_triangulated),
                    pnp_op=np.array(self.pnp_op, dtype=np.int32)[:F], pnp_count=np.array(self.pnp_count, dtype=np.int32)[:F],
                    pnp=[self.pnp[f].as_dict() for f in range(F)])


SFM_MIN_PNP = 10  # solveFrameByPnP returns false below it (initial_sfm.cpp:51-52)


class RelativePoseInC(C.Structure):
    """LfvioRelativePoseIn (include/lfvio.h)."""
    _fields_ = [
        ("num_pairs", C.c_int),
        ("match_offset", C.POINTER(C.c_int)),
        ("bearing_l", C.POINTER(C.c_double)),
        ("bearing_r", C.POINTER(C.c_double)),
        ("num_samples", C.c_int),
        ("samples", C.POINTER(C.c_int)),
    ]


class RelativePosePairC(C.Structure):
    """LfvioRelativePosePair (include/lfvio.h)."""
    _fields_ = [
        ("gate", C.c_int),
        ("num_matches", C.c_int),
        ("best_sample", C.c_int),
        ("num_inliers", C.c_int),
        ("average_parallax", C.c_double),
        ("best_score", C.c_double),
        ("E", C.c_double * 9),
        ("R_cand", (C.c_double * 9) * 2),
        ("t_cand", C.c_double * 3),
        ("good", C.c_int * 4),
        ("chosen", C.c_int),
        ("inlier_cnt", C.c_int),
        ("ok", C.c_int),
        ("pad_", C.c_int),
        ("rot", C.c_double * 9),
        ("trans", C.c_double * 3),
        ("rotation", C.c_double * 9),
        ("translation", C.c_double * 3),
    ]

    def as_dict(self):
        a = lambda x: np.array(x, dtype=np.float64)
        return dict(gate=int(self.gate), num_matches=int(self.num_matches), best_sample=int(self.best_sample), num_inliers=int(self.num_inliers),
                    average_parallax=float(self.average_parallax), best_score=float(self.best_score), E=a(self.E),
                    R_cand=np.array([list(self.R_cand[0]), list(self.R_cand[1])]).reshape(2, 3, 3), t_cand=a(self.t_cand),
                    good=np.array(self.good, dtype=np.int32), chosen=int(self.chosen), inlier_cnt=int(self.inlier_cnt), ok=int(self.ok),
                    rot=a(self.rot).reshape(3, 3), trans=a(self.trans), rotation=a(self.rotation).reshape(3, 3), translation=a(self.translation))


class RelativePoseOutC(C.Structure):
    """LfvioRelativePoseOut (include/lfvio.h)."""
    _fields_ = [
        ("l", C.c_int),
        ("pad_", C.c_int),
        ("relative_R", C.c_double * 9),
        ("relative_T", C.c_double * 3),
        ("pair", RelativePosePairC * WINDOW_SIZE),
    ]

    def as_dict(self, P=WINDOW_SIZE):
        return dict(l=int(self.l), relative_R=np.array(self.relative_R, dtype=np.float64).reshape(3, 3), relative_T=np.array(self.relative_T, dtype=np.float64),
                    pair=[self.pair[p].as_dict() for p in range(P)])


class KltInC(C.Structure):
    """LfvioKltIn (include/lfvio.h)."""
    _fields_ = [
        ("width", C.c_int),
        ("height", C.c_int),
        ("image", C.POINTER(C.c_ubyte)),
        ("num_points", C.c_int),
        ("prev_pts", C.POINTER(C.c_float)),
        ("win_size", C.c_int),
        ("max_level", C.c_int),
        ("max_iterations", C.c_int),
        ("epsilon", C.c_double),
        ("min_eig_threshold", C.c_double),
        ("border", C.c_int),
    ]


class KltOutC(C.Structure):
    """LfvioKltOut (include/lfvio.h)."""
    _fields_ = [("levels_used", C.c_int), ("num_tracked", C.c_int)]


KLT_MAX_POINTS, KLT_MAX_LEVEL = 4096, 5  # LFVIO_KLT_MAX_POINTS, LFVIO_KLT_MAX_LEVEL


class GftInC(C.Structure):
    """LfvioGftIn (include/lfvio.h)."""
    _fields_ = [
        ("num_points", C.c_int),
        ("pts", C.POINTER(C.c_float)),
        ("track_cnt", C.POINTER(C.c_int)),
        ("max_count", C.c_int),
        ("quality_level", C.c_double),
        ("min_distance", C.c_int),
        ("mask_radius", C.c_int),
    ]


class GftOutC(C.Structure):
    """LfvioGftOut (include/lfvio.h)."""
    _fields_ = [("num_kept", C.c_int), ("num_corners", C.c_int), ("num_candidates", C.c_int), ("max_response", C.c_double)]


GFT_MAX_CORNERS = 4096  # LFVIO_GFT_MAX_CORNERS


class ClaheInC(C.Structure):
    """LfvioClaheIn (include/lfvio.h)."""
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)]


CLAHE_MAX_TILES = 16  # LFVIO_CLAHE_MAX_TILES


class ImageFormatC(C.Structure):
    """LfvioImageFormat (include/lfvio.h)."""
    _fields_ = [("encoding", C.c_int), ("step", C.c_int)]


# LFVIO_IMG_*: the encodings of lfvio_image_format_set and of the type-10 record
IMG_MONO8, IMG_BGR8, IMG_RGB8, IMG_BGRA8, IMG_RGBA8, IMG_MONO16, IMG_MONO16_BE = 0, 2, 3, 4, 5, 6, 7
IMG_BPP = {IMG_MONO8: 1, IMG_BGR8: 3, IMG_RGB8: 3, IMG_BGRA8: 4, IMG_RGBA8: 4, IMG_MONO16: 2, IMG_MONO16_BE: 2}
IMG_MAX_STEP = 65536  # LFVIO_IMG_MAX_STEP


class CameraC(C.Structure):
    """LfvioCamera (include/lfvio.h).  The fields behind poly are PINHOLE's and MEI's; positional construction with the eleven
    values of an OCam camera leaves them zero."""
    _fields_ = [("model", C.c_int), ("cx", C.c_double), ("cy", C.c_double), ("c", C.c_double), ("d", C.c_double), ("e", C.c_double),
                ("poly", C.c_double * 5), ("fx", C.c_double), ("fy", C.c_double), ("k1", C.c_double), ("k2", C.c_double),
                ("p1", C.c_double), ("p2", C.c_double), ("xi", C.c_double)]


class TrackRejectInC(C.Structure):
    """LfvioTrackRejectIn (include/lfvio.h)."""
    _fields_ = [
        ("camera", C.POINTER(CameraC)),
        ("num_points", C.c_int),
        ("cur_pts", C.POINTER(C.c_float)),
        ("forw_pts", C.POINTER(C.c_float)),
        ("num_samples", C.c_int),
        ("samples", C.POINTER(C.c_int)),
    ]


class TrackRejectOutC(C.Structure):
    """LfvioTrackRejectOut (include/lfvio.h)."""
    _fields_ = [("status", C.c_int), ("best_sample", C.c_int), ("num_inliers", C.c_int), ("best_score", C.c_double), ("E", C.c_double * 9)]


class TrackUndistortInC(C.Structure):
    """LfvioTrackUndistortIn (include/lfvio.h)."""
    _fields_ = [("camera", C.POINTER(CameraC)), ("num_points", C.c_int), ("pts", C.POINTER(C.c_float)), ("ids", C.POINTER(C.c_int)),
                ("time", C.c_double)]


CAM_OCAM, TRACK_MAX_POINTS = 0, 4096  # LFVIO_CAM_OCAM, LFVIO_TRACK_MAX_POINTS
CAM_PINHOLE, CAM_MEI = 2, 3  # LFVIO_CAM_PINHOLE, LFVIO_CAM_MEI
CAM_KANNALA_BRANDT = 5  # LFVIO_CAM_KANNALA_BRANDT
CAM_EQUIRECT = 6  # LFVIO_CAM_EQUIRECT: the lift only; fx, fy = the expanded image's width, height


def camera_c(cam):
    """A CameraC from a camera dict.  model (optional) LFVIO_CAM_OCAM: cx, cy, c, d, e, poly [5]; LFVIO_CAM_PINHOLE: cx, cy, fx, fy,
    k1, k2, p1, p2; LFVIO_CAM_MEI: those (u0, v0, gamma1, gamma2 under cx, cy, fx, fy) and xi; LFVIO_CAM_KANNALA_BRANDT: cx, cy, fx, fy
    (u0, v0, mu, mv) and k2, k3, k4, k5, which go into poly[0 .. 3] and NOT into the struct's k1, k2; LFVIO_CAM_EQUIRECT: fx, fy, the
    expanded image's width and height.  The fields of the other models may be left out (zero)."""
    g = lambda k: float(cam.get(k, 0.0))
    model = int(cam.get("model", CAM_OCAM))
    if model == CAM_EQUIRECT:  # fx, fy (the image's width and height) alone
        return CameraC(model, g("cx"), g("cy"), 0.0, 0.0, 0.0, (C.c_double * 5)(), g("fx"), g("fy"))
    if model == CAM_KANNALA_BRANDT:
        return CameraC(model, cam["cx"], cam["cy"], 0.0, 0.0, 0.0, (C.c_double * 5)(g("k2"), g("k3"), g("k4"), g("k5"), 0.0), g("fx"), g("fy"))
    return CameraC(model, cam["cx"], cam["cy"], g("c"), g("d"), g("e"), (C.c_double * 5)(*[float(v) for v in cam.get("poly", (0.0,) * 5)]),
                   g("fx"), g("fy"), g("k1"), g("k2"), g("p1"), g("p2"), g("xi"))


OCAM_INV_POLY_SIZE = 20  # LFVIO_OCAM_INV_POLY_SIZE
MAP_EQUIRECT, MAP_PERSPECTIVE = 0, 1  # LFVIO_MAP_*
CAM_PROJECT_MAX_POINTS = 1 << 20


class ProjectorC(C.Structure):
    """LfvioProjector (include/lfvio.h)."""
    _fields_ = [("camera", C.POINTER(CameraC)), ("inv_poly", C.c_double * OCAM_INV_POLY_SIZE)]


class RemapInC(C.Structure):
    """LfvioRemapIn (include/lfvio.h)."""
    _fields_ = [("proj", C.POINTER(ProjectorC)), ("kind", C.c_int), ("width", C.c_int), ("height", C.c_int), ("M", C.c_double * 9)]


def projector_c(cam):
    """(ProjectorC, CameraC) from a camera dict (camera_c); an OCam camera's `inv_poly` (up to 20 numbers) fills the inverse
    polynomial, the tail is 0.0.  The CameraC is returned to keep it alive beside the pointer."""
    cc = cam if isinstance(cam, CameraC) else camera_c(cam)
    inv = [float(v) for v in (() if isinstance(cam, CameraC) else cam.get("inv_poly", ()))]
    return ProjectorC(C.pointer(cc), (C.c_double * OCAM_INV_POLY_SIZE)(*inv)), cc


class TrackSourceC(C.Structure):
    """LfvioTrackSource (include/lfvio.h)."""
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int)]


FUSE_EQUIRECT, FUSE_CAMERA = 0, 1  # LFVIO_FUSE_*
FUSE_IMAGE_NONE, FUSE_IMAGE_GIVEN, FUSE_IMAGE_REMAP = 0, 1, 2  # LFVIO_FUSE_IMAGE_*
FUSE_MAX_POINTS = 1 << 20


class FuseInC(C.Structure):
    """LfvioFuseIn (include/lfvio.h)."""
    _fields_ = [("cloud", C.POINTER(C.c_ubyte)), ("n", C.c_int), ("point_step", C.c_int), ("off_x", C.c_int), ("off_y", C.c_int), ("off_z", C.c_int),
                ("big_endian", C.c_int), ("R", C.c_double * 9), ("T", C.c_double * 3), ("min_range", C.c_double), ("max_range", C.c_double),
                ("kind", C.c_int), ("width", C.c_int), ("height", C.c_int), ("proj", C.POINTER(ProjectorC)), ("image_mode", C.c_int),
                ("fmt", C.POINTER(ImageFormatC)), ("src_width", C.c_int), ("src_height", C.c_int), ("pixels", C.POINTER(C.c_ubyte)),
                ("paint_on", C.c_int), ("paint", C.c_ubyte * 4)]


class FuseOutC(C.Structure):
    """LfvioFuseOut (include/lfvio.h): each pointer null, or written."""
    _fields_ = [("index", C.POINTER(C.c_int)), ("range", C.POINTER(C.c_float)), ("colour", C.POINTER(C.c_ubyte)), ("image_out", C.POINTER(C.c_ubyte)),
                ("counts", C.POINTER(C.c_int))]


class TrackFrameInC(C.Structure):
    """LfvioTrackFrameIn (include/lfvio.h)."""
    _fields_ = [
        ("width", C.c_int),
        ("height", C.c_int),
        ("image", C.POINTER(C.c_ubyte)),
        ("time", C.c_double),
        ("publish", C.c_int),
        ("camera", C.POINTER(CameraC)),
        ("win_size", C.c_int),
        ("max_level", C.c_int),
        ("max_iterations", C.c_int),
        ("epsilon", C.c_double),
        ("min_eig_threshold", C.c_double),
        ("border", C.c_int),
        ("max_count", C.c_int),
        ("quality_level", C.c_double),
        ("min_distance", C.c_int),
        ("mask_radius", C.c_int),
        ("num_samples", C.c_int),
        ("sample_words", C.POINTER(C.c_uint)),
        ("capacity", C.c_int),
    ]


class TrackFrameOutC(C.Structure):
    """LfvioTrackFrameOut (include/lfvio.h)."""
    _fields_ = [
        ("num_points", C.c_int),
        ("num_new", C.c_int),
        ("levels_used", C.c_int),
        ("num_tracked", C.c_int),
        ("num_after_reject", C.c_int),
        ("reject", TrackRejectOutC),
        ("detect", GftOutC),
        ("pts", C.POINTER(C.c_float)),
        ("ids", C.POINTER(C.c_int)),
        ("track_cnt", C.POINTER(C.c_int)),
        ("un_pts", C.POINTER(C.c_float)),
        ("un_pts_3d", C.POINTER(C.c_float)),
        ("velocity_3d", C.POINTER(C.c_float)),
    ]


class TrackFrameStagesC(C.Structure):
    """LfvioTrackFrameStages (include/lfvio.h)."""
    _fields_ = [
        ("next_pts", C.POINTER(C.c_float)),
        ("status", C.POINTER(C.c_ubyte)),
        ("samples", C.POINTER(C.c_int)),
        ("mask", C.POINTER(C.c_ubyte)),
        ("kept", C.POINTER(C.c_int)),
        ("corners", C.POINTER(C.c_float)),
    ]


class TrackMessageC(C.Structure):
    """LfvioTrackMessage (include/lfvio.h)."""
    _fields_ = [("num_rows", C.c_int), ("rows", C.POINTER(C.c_float))]


RELPOSE_MIN_MATCHES = 20  # a pair runs when N > 20 (estimator.cpp:452)

HIP_SYMBOLS = [
    "lfvio_create", "lfvio_destroy", "lfvio_last_error", "lfvio_version", "lfvio_solve", "lfvio_solve_relo", "lfvio_marginalize",
    "lfvio_batch_reserve", "lfvio_batch_upload", "lfvio_batch_optimize", "lfvio_batch_optimize_async",
    "lfvio_batch_sync", "lfvio_batch_download", "lfvio_stream",
    "lfvio_batch_optimize_begin", "lfvio_batch_optimize_finish", "lfvio_batch_optimize_pending", "lfvio_batch_upload_chained", "lfvio_batch_upload_chained_device",
    "lfvio_shard_begin", "lfvio_shard_exchange_len", "lfvio_shard_scalar_offset", "lfvio_shard_exchange_ptr", "lfvio_shard_linearize",
    "lfvio_shard_solve", "lfvio_shard_candidate", "lfvio_shard_decide", "lfvio_shard_marg_linearize", "lfvio_shard_marg_finish",
    "lfvio_shard_finish", "lfvio_shard_restart", "lfvio_shard_enqueue", "lfvio_shard_poll", "lfvio_triangulate", "lfvio_shift_depth", "lfvio_preintegrate",
    "lfvio_two_view", "lfvio_vi_align", "lfvio_pnp", "lfvio_sfm_ba", "lfvio_sfm_construct", "lfvio_relative_pose",
    "lfvio_klt_track", "lfvio_klt_reset", "lfvio_klt_level", "lfvio_gft_detect", "lfvio_gft_set_mask", "lfvio_gft_response",
    "lfvio_clahe_set", "lfvio_clahe_apply", "lfvio_image_format_set", "lfvio_image_gray", "lfvio_track_batch_format",
    "lfvio_track_reject", "lfvio_track_undistort", "lfvio_track_reset", "lfvio_track_frame", "lfvio_track_frame_reset",
    "lfvio_track_frame_message",
    "lfvio_cam_project", "lfvio_remap_build", "lfvio_remap_apply", "lfvio_remap_reset", "lfvio_cloud_fuse",
    "lfvio_track_source_set",
    "lfvio_track_batch_reserve", "lfvio_track_batch_set_mask", "lfvio_track_batch_clahe", "lfvio_track_batch_frame", "lfvio_track_batch_reset",
    "lfvio_track_batch_map", "lfvio_track_batch_source", "lfvio_track_batch_level",
    "lfvio_group_create", "lfvio_group_unique_id", "lfvio_group_create_rank", "lfvio_group_create_local", "lfvio_group_destroy",
    "lfvio_group_last_error", "lfvio_group_size", "lfvio_group_local", "lfvio_group_rank", "lfvio_group_ctx", "lfvio_group_backend",
    "lfvio_group_solve", "lfvio_group_upload", "lfvio_group_optimize", "lfvio_group_download", "lfvio_group_range",
    "lfvio_group_last_passes", "lfvio_group_last_collectives", "lfvio_group_payload_doubles", "lfvio_group_batch_reserve", "lfvio_group_batch_upload",
    "lfvio_group_batch_optimize", "lfvio_group_batch_download",
]


def load_hip_library(path=None):
    """dlopen the product library.  No fallback: a missing build is an error."""
    path = path or HIP_LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (hipcc, gfx950); "
                           "there is no CPU fallback for the product path")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; the dynamic linker de-duplicates by soname, so
    # whichever HIP runtime is loaded FIRST serves both.  torch cannot run on a foreign runtime ("No HIP GPUs
    # are available"), while this library is happy on torch's — so when torch is part of the process (bench,
    # sharded tests: device pointers are shared with torch.distributed/RCCL) it must be loaded first.
    try:
        import torch  # noqa: F401
        torch.cuda.is_available()
    except ImportError:
        pass
    lib = C.CDLL(path)
    lib.lfvio_create.restype = C.c_void_p
    lib.lfvio_create.argtypes = [C.c_int]
    lib.lfvio_destroy.argtypes = [C.c_void_p]
    lib.lfvio_destroy.restype = None
    lib.lfvio_last_error.restype = C.c_char_p
    lib.lfvio_last_error.argtypes = [C.c_void_p]
    lib.lfvio_version.restype = C.c_char_p
    lib.lfvio_solve.argtypes = [C.c_void_p, C.POINTER(WindowC), C.POINTER(SolutionC)]
    lib.lfvio_solve_relo.argtypes = [C.c_void_p, C.POINTER(WindowC), C.POINTER(ReloC), C.POINTER(SolutionC), C.POINTER(C.c_double)]
    lib.lfvio_marginalize.argtypes = [C.c_void_p, C.POINTER(WindowC), C.c_int, C.POINTER(Prior)]
    lib.lfvio_batch_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.lfvio_batch_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(WindowC)]
    lib.lfvio_batch_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lfvio_batch_optimize_async.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lfvio_batch_sync.argtypes = [C.c_void_p]
    lib.lfvio_batch_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(SolutionC), C.POINTER(Prior)]
    lib.lfvio_batch_optimize_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(SolutionC)]
    lib.lfvio_batch_optimize_finish.argtypes = [C.c_void_p, C.POINTER(Prior)]
    lib.lfvio_batch_optimize_pending.argtypes = [C.c_void_p]
    lib.lfvio_batch_upload_chained.argtypes = [C.c_void_p, C.c_int, C.POINTER(WindowC), C.POINTER(Prior)]
    lib.lfvio_batch_upload_chained_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(WindowC)]
    lib.lfvio_stream.restype = C.c_void_p
    lib.lfvio_stream.argtypes = [C.c_void_p]
    lib.lfvio_shard_begin.argtypes = [C.c_void_p, C.POINTER(WindowC), C.c_int, C.c_int, C.c_int]
    lib.lfvio_shard_exchange_len.restype = C.c_int
    lib.lfvio_shard_scalar_offset.restype = C.c_int
    lib.lfvio_shard_exchange_ptr.restype = C.c_void_p
    lib.lfvio_shard_exchange_ptr.argtypes = [C.c_void_p]
    for name in ("lfvio_shard_linearize", "lfvio_shard_solve", "lfvio_shard_candidate"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.lfvio_shard_decide.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.lfvio_shard_restart.argtypes = [C.c_void_p]
    lib.lfvio_shard_enqueue.argtypes = [C.c_void_p, C.c_int]
    lib.lfvio_shard_poll.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.lfvio_shard_finish.argtypes = [C.c_void_p, C.POINTER(SolutionC)]
    _dp = C.POINTER(C.c_double)
    lib.lfvio_triangulate.argtypes = [C.c_void_p, C.POINTER(TriangulateInC), _dp]
    lib.lfvio_shift_depth.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp]
    lib.lfvio_preintegrate.argtypes = [C.c_void_p, C.c_int, C.POINTER(ImuIntervalC), _dp, C.POINTER(Preintegration)]
    lib.lfvio_two_view.argtypes = [C.c_void_p, C.POINTER(TwoViewInC), C.POINTER(C.c_ubyte), C.POINTER(TwoViewOutC), _dp, C.POINTER(C.c_float)]
    if hasattr(lib, "lfvio_vi_align"):  # (an A/B run may load a build from before the entry existed; build() checks the product's symbols)
        lib.lfvio_vi_align.argtypes = [C.c_void_p, C.POINTER(ViAlignInC), C.POINTER(ViAlignOutC), _dp, C.POINTER(Preintegration)]
    if hasattr(lib, "lfvio_pnp"):
        lib.lfvio_pnp.argtypes = [C.c_void_p, C.POINTER(PnpInC), C.POINTER(PnpOutC)]
    if hasattr(lib, "lfvio_sfm_ba"):
        lib.lfvio_sfm_ba.argtypes = [C.c_void_p, C.POINTER(SfmBaInC), _dp, _dp, _dp, C.POINTER(SfmBaOutC)]
    if hasattr(lib, "lfvio_sfm_construct"):
        lib.lfvio_sfm_construct.argtypes = [C.c_void_p, C.POINTER(SfmConstructInC), _dp, _dp, _dp, C.POINTER(C.c_int), C.POINTER(SfmConstructOutC)]
    if hasattr(lib, "lfvio_relative_pose"):
        lib.lfvio_relative_pose.argtypes = [C.c_void_p, C.POINTER(RelativePoseInC), C.POINTER(C.c_ubyte), C.POINTER(RelativePoseOutC)]
    if hasattr(lib, "lfvio_klt_track"):
        lib.lfvio_klt_track.argtypes = [C.c_void_p, C.POINTER(KltInC), C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int), C.POINTER(KltOutC)]
        lib.lfvio_klt_reset.argtypes = [C.c_void_p]
        lib.lfvio_klt_level.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
    if hasattr(lib, "lfvio_gft_detect"):
        lib.lfvio_gft_detect.argtypes = [C.c_void_p, C.POINTER(GftInC), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(GftOutC)]
        lib.lfvio_gft_set_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]
        lib.lfvio_gft_response.argtypes = [C.c_void_p, _dp]
    if hasattr(lib, "lfvio_clahe_set"):
        lib.lfvio_clahe_set.argtypes = [C.c_void_p, C.POINTER(ClaheInC)]
        lib.lfvio_clahe_apply.argtypes = [C.c_void_p, C.POINTER(ClaheInC), C.c_int, C.c_int] + [C.POINTER(C.c_ubyte)] * 3
    if hasattr(lib, "lfvio_image_format_set"):
        lib.lfvio_image_format_set.argtypes = [C.c_void_p, C.POINTER(ImageFormatC)]
        lib.lfvio_image_gray.argtypes = [C.c_void_p, C.POINTER(ImageFormatC), C.c_int, C.c_int] + [C.POINTER(C.c_ubyte)] * 2
        lib.lfvio_track_batch_format.argtypes = [C.c_void_p, C.POINTER(ImageFormatC)]
    if hasattr(lib, "lfvio_cam_project"):
        lib.lfvio_cam_project.argtypes = [C.c_void_p, C.POINTER(ProjectorC), C.c_int, _dp, _dp]
        lib.lfvio_remap_build.argtypes = [C.c_void_p, C.POINTER(RemapInC), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.lfvio_remap_apply.argtypes = [C.c_void_p, C.POINTER(ImageFormatC), C.c_int, C.c_int] + [C.POINTER(C.c_ubyte)] * 2
        lib.lfvio_remap_reset.argtypes = [C.c_void_p]
    if hasattr(lib, "lfvio_track_source_set"):
        lib.lfvio_track_source_set.argtypes = [C.c_void_p, C.POINTER(TrackSourceC)]
    if hasattr(lib, "lfvio_cloud_fuse"):
        lib.lfvio_cloud_fuse.argtypes = [C.c_void_p, C.POINTER(FuseInC), C.POINTER(FuseOutC)]
    if hasattr(lib, "lfvio_track_reject"):
        lib.lfvio_track_reject.argtypes = [C.c_void_p, C.POINTER(TrackRejectInC), C.POINTER(C.c_ubyte), C.POINTER(TrackRejectOutC), _dp, _dp]
        lib.lfvio_track_undistort.argtypes = [C.c_void_p, C.POINTER(TrackUndistortInC)] + [C.POINTER(C.c_float)] * 3 + [C.POINTER(C.c_int)]
        lib.lfvio_track_reset.argtypes = [C.c_void_p]
    if hasattr(lib, "lfvio_track_frame"):
        lib.lfvio_track_frame.argtypes = [C.c_void_p, C.POINTER(TrackFrameInC), C.POINTER(TrackFrameOutC), C.POINTER(TrackFrameStagesC)]
        lib.lfvio_track_frame_reset.argtypes = [C.c_void_p]
    if hasattr(lib, "lfvio_track_frame_message"):
        lib.lfvio_track_frame_message.argtypes = [C.c_void_p, C.POINTER(TrackFrameInC), C.POINTER(TrackFrameOutC), C.POINTER(TrackFrameStagesC),
                                                  C.POINTER(TrackMessageC)]
    if hasattr(lib, "lfvio_track_batch_frame"):
        lib.lfvio_track_batch_reserve.argtypes = [C.c_void_p, C.c_int]
        lib.lfvio_track_batch_set_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]
        lib.lfvio_track_batch_clahe.argtypes = [C.c_void_p, C.POINTER(ClaheInC)]
        lib.lfvio_track_batch_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(TrackFrameInC), C.POINTER(TrackFrameOutC), C.POINTER(TrackMessageC)]
        lib.lfvio_track_batch_reset.argtypes = [C.c_void_p, C.c_int]
    if hasattr(lib, "lfvio_track_batch_map"):
        lib.lfvio_track_batch_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(RemapInC)]
        lib.lfvio_track_batch_source.argtypes = [C.c_void_p, C.POINTER(TrackSourceC)]
        lib.lfvio_track_batch_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
    lib.lfvio_shard_marg_linearize.argtypes = [C.c_void_p, C.c_int]
    lib.lfvio_shard_marg_finish.argtypes = [C.c_void_p, C.c_int, C.POINTER(Prior)]
    # multi-GPU groups (RCCL inside the library)
    lib.lfvio_group_create.restype = C.c_void_p
    lib.lfvio_group_create.argtypes = [C.c_uint]
    lib.lfvio_group_unique_id.argtypes = [C.c_char_p]
    lib.lfvio_group_create_rank.restype = C.c_void_p
    lib.lfvio_group_create_rank.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.lfvio_group_create_local.restype = C.c_void_p
    lib.lfvio_group_create_local.argtypes = [C.c_int, C.c_int]
    lib.lfvio_group_destroy.argtypes = [C.c_void_p]
    lib.lfvio_group_destroy.restype = None
    lib.lfvio_group_last_error.restype = C.c_char_p
    lib.lfvio_group_last_error.argtypes = [C.c_void_p]
    lib.lfvio_group_backend.restype = C.c_char_p
    lib.lfvio_group_backend.argtypes = [C.c_void_p]
    for name in ("lfvio_group_size", "lfvio_group_local", "lfvio_group_rank", "lfvio_group_last_passes", "lfvio_group_last_collectives"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.lfvio_group_ctx.restype = C.c_void_p
    lib.lfvio_group_ctx.argtypes = [C.c_void_p, C.c_int]
    lib.lfvio_group_solve.argtypes = [C.c_void_p, C.POINTER(WindowC), C.c_int, C.POINTER(SolutionC), C.POINTER(Prior)]
    lib.lfvio_group_upload.argtypes = [C.c_void_p, C.POINTER(WindowC)]
    lib.lfvio_group_optimize.argtypes = [C.c_void_p, C.c_int]
    lib.lfvio_group_download.argtypes = [C.c_void_p, C.POINTER(SolutionC), C.POINTER(Prior)]
    lib.lfvio_group_range.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.lfvio_group_batch_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.lfvio_group_batch_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(WindowC)]
    lib.lfvio_group_batch_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lfvio_group_batch_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(SolutionC), C.POINTER(Prior)]
    return lib


# ---------------------------------------------------------------------------
# (de)serialisation of windows / priors to plain numpy dicts (fixtures, traces)
# ---------------------------------------------------------------------------
def preint_to_array(pre):
    return np.concatenate([[pre.sum_dt], pre.delta_p[:], pre.delta_q[:], pre.delta_v[:], pre.linearized_ba[:],
                           pre.linearized_bg[:], pre.jacobian[:], pre.covariance[:]])


def preint_from_array(a):
    pre = Preintegration()
    a = np.asarray(a, dtype=np.float64)
    pre.sum_dt = a[0]
    o = 1
    for name, n in (("delta_p", 3), ("delta_q", 4), ("delta_v", 3), ("linearized_ba", 3), ("linearized_bg", 3),
                    ("jacobian", 225), ("covariance", 225)):
        arr = getattr(pre, name)
        for k in range(n):
            arr[k] = a[o + k]
        o += n
    return pre


def prior_to_dict(p, prefix="prior_"):
    if p is None or not p.valid:
        return {prefix + "valid": np.array(0)}
    nb = p.num_blocks
    return {
        prefix + "valid": np.array(1), prefix + "m": np.array(p.m), prefix + "n": np.array(p.n),
        prefix + "blocks": np.array([[p.blocks[i].kind, p.blocks[i].frame, p.block_idx[i]] for i in range(nb)]),
        prefix + "x0": np.array([p.block_x0[i][:] for i in range(nb)]),
        prefix + "J": p.J(), prefix + "r": p.r(),
    }


def prior_from_dict(d, prefix="prior_"):
    if int(d[prefix + "valid"]) == 0:
        return None
    p = Prior()
    p.valid = 1
    p.m, p.n = int(d[prefix + "m"]), int(d[prefix + "n"])
    blocks = np.asarray(d[prefix + "blocks"])
    p.num_blocks = blocks.shape[0]
    x0 = np.asarray(d[prefix + "x0"])
    for i in range(p.num_blocks):
        p.blocks[i].kind, p.blocks[i].frame, p.block_idx[i] = int(blocks[i, 0]), int(blocks[i, 1]), int(blocks[i, 2])
        for k in range(9):
            p.block_x0[i][k] = x0[i, k]
    J = np.asarray(d[prefix + "J"], dtype=np.float64).reshape(-1)
    r = np.asarray(d[prefix + "r"], dtype=np.float64)
    C.memmove(p.linearized_jacobians, J.ctypes.data, J.nbytes)
    C.memmove(p.linearized_residuals, r.ctypes.data, r.nbytes)
    return p


def window_to_dict(w):
    d = dict(pose=w.pose, speed_bias=w.speed_bias, ex_pose=w.ex_pose, td=np.array(w.td), start_frame=w.start_frame,
             obs_offset=w.obs_offset, inv_depth=w.inv_depth, obs_point=w.obs_point, obs_velocity=w.obs_velocity,
             obs_cur_td=w.obs_cur_td, obs_uv_y=w.obs_uv_y, imu=np.array([preint_to_array(p) for p in w.imu]),
             flags=np.array([w.estimate_extrinsic, w.estimate_td, w.max_num_iterations]),
             consts=np.array([w.max_solver_time, w.g[0], w.g[1], w.g[2], w.tr, w.row, w.sqrt_info]))
    d.update(prior_to_dict(w.prior))
    return d


def window_from_dict(d):
    fl, cs = np.asarray(d["flags"]), np.asarray(d["consts"])
    return Window(d["pose"], d["speed_bias"], d["ex_pose"], float(d["td"]), d["start_frame"], d["obs_offset"],
                  d["inv_depth"], d["obs_point"], d["obs_velocity"], d["obs_cur_td"], d["obs_uv_y"],
                  [preint_from_array(a) for a in np.asarray(d["imu"])], prior=prior_from_dict(d),
                  estimate_extrinsic=int(fl[0]), estimate_td=int(fl[1]), max_num_iterations=int(fl[2]),
                  max_solver_time=float(cs[0]), g=(cs[1], cs[2], cs[3]), tr=float(cs[4]), row=float(cs[5]),
                  sqrt_info=float(cs[6]))
