"""Thin object wrapper over the C-ABI of liblfvio_hip.so (no compute, no fallback)."""
import ctypes as C

import numpy as np

from . import abi

_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def annulus_mask(w, h, cx, cy, max_r, min_r):
    """The base mask of feature_tracker.cpp:53-56 as a [h, w] uint8 array for Engine.gft_set_mask: 255 where min_r^2 < (x - cx)^2 +
    (y - cy)^2 <= max_r^2, 0 elsewhere.  Euclidean discs: cv::circle rasterises its own, which differ in a few rim pixels."""
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    return np.where((d2 <= max_r * max_r) & (d2 > min_r * min_r), 255, 0).astype(np.uint8)


class Engine:
    def __init__(self, device=0, lib_path=None):
        self.lib = abi.load_hip_library(lib_path)
        self.lib.lfvio_debug_linearize.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), _dp, _dp, _dp, _dp, _dp, _dp]
        self.lib.lfvio_debug_marg_system.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        self.lib.lfvio_debug_configure.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        self.lib.lfvio_debug_query.argtypes = [C.c_void_p, C.c_char_p, _dp, C.c_int]
        self.lib.lfvio_debug_time_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        self.lib.lfvio_debug_pass_io.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(Engine._PassIO)]
        self.lib.lfvio_debug_step_io.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(Engine._StepIO)]
        self.lib.lfvio_debug_schur_repeat.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_double, _dp]
        self.ctx = self.lib.lfvio_create(device)
        if not self.ctx:
            raise RuntimeError("lfvio_create failed: no usable HIP device (there is no CPU fallback)")

    def close(self):
        if self.ctx:
            self.lib.lfvio_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}: {self.lib.lfvio_last_error(self.ctx).decode()}")

    # ---- the debug interface (include/lfvio_debug.h): every switch is a key of lfvio_debug_configure, every counter one of lfvio_debug_query
    def configure(self, key, value=1.0):
        self._check(self.lib.lfvio_debug_configure(self.ctx, key.encode(), float(value)), f"lfvio_debug_configure({key})")

    def query(self, key, n, first=0.0):
        out = np.zeros(max(n, 1))
        out[0] = first
        self._check(self.lib.lfvio_debug_query(self.ctx, key.encode(), _p(out), n), f"lfvio_debug_query({key})")
        return out

    def set_graph(self, on):
        self.configure("graph", int(on))

    def marg_ahead(self, on=-1):
        """on = 0 / 1: the windows uploaded from now on end with the serial tail / may have their marginalization started on worker
        streams as soon as a state is accepted (csrc/kernels_spec.h; -1: leave).  Returns (calls with workers, priors a worker delivered)."""
        if on >= 0:
            self.configure("marg_ahead", int(on))
        q = self.query("marg_ahead", 2)
        return int(q[0]), int(q[1])

    def break_next_chain(self):
        self.configure("break_next_chain", 1)

    def set_lm_half(self, on):
        self.configure("lm_half", int(on))

    def set_initial_radius(self, r):
        self.configure("initial_radius", float(r))

    def set_linw(self, mode):
        """How resident batches are linearized (include/lfvio_debug.h): 1 default, 0 never k_linw, 2 every launch of planned windows."""
        self.configure("linw", int(mode))

    def resident_pass(self, count, slot, n_landmarks):
        """One linearization + dense solve of the resident slots; what it left in `slot`: a view on pass_io (lm_sum: its first 5)."""
        io = self.pass_io(count, slot, n_landmarks)
        return dict({k: io[k] for k in ("gp", "schur", "a", "b", "gn_p", "q", "linw")}, lm_sum=io["lm_sum"][:5], x_cost=np.array([io["x_cost"]]))

    class _PassIO(C.Structure):  # LfvioPassIO of include/lfvio_debug.h
        _ARRAYS = ("H", "gp", "schur", "lm_sum", "imu_out", "prior_A", "prior_cmap", "a", "b", "W",
                   "scale_p", "diag_p", "grad_p", "gn_p", "uc_grad", "uc_gn", "q")
        _fields_ = ([(k, C.POINTER(C.c_int) if k == "prior_cmap" else _dp) for k in _ARRAYS]
                    + [(k, C.c_double) for k in ("alpha", "grad_sq_total", "x_cost", "mu", "prior_cost")]
                    + [(k, C.c_int) for k in ("chol_fail", "prior_n", "est_ex", "est_td", "num_landmarks")])

    @staticmethod
    def _pass_buffers(N):
        """The seventeen arrays of LfvioPassIO for a slot of N landmarks."""
        KP, n1 = abi.KP, max(N, 1)
        return dict(H=np.zeros(KP * (KP + 1) // 2), gp=np.zeros(KP), schur=np.zeros(15 * 256), lm_sum=np.zeros(16), imu_out=np.zeros((10, 932)),
                    prior_A=np.zeros(KP * KP), prior_cmap=np.zeros(KP, np.int32), a=np.zeros(n1), b=np.zeros(n1),
                    W=np.zeros((n1, abi.KC)), scale_p=np.zeros(KP), diag_p=np.zeros(KP), grad_p=np.zeros(KP), gn_p=np.zeros(KP),
                    uc_grad=np.zeros(80), uc_gn=np.zeros(80), q=np.zeros(16))

    @staticmethod
    def _bind_pass(io_struct, out):
        for k in Engine._PassIO._ARRAYS:
            setattr(io_struct, k, out[k].ctypes.data_as(C.POINTER(C.c_int) if k == "prior_cmap" else _dp))

    @staticmethod
    def _pass_result(ps, out, N, rc):
        """`out` trimmed to the sizes the library reports in `ps` (a _PassIO), with its scalars and the sweep kernel `rc`."""
        n = ps.prior_n
        out.update(a=out["a"][:N], b=out["b"][:N], W=out["W"][:N], prior_A=out["prior_A"][:n * n].reshape(n, n).copy(),
                   prior_cmap=out["prior_cmap"][:n].copy(), linw=rc)
        for k in ("alpha", "grad_sq_total", "x_cost", "mu", "prior_cost", "chol_fail", "prior_n", "est_ex", "est_td"):
            out[k] = getattr(ps, k)
        return out

    def pass_io(self, count, slot, n_landmarks, mu=0.0):
        """One linearization + dense solve of the resident slots [0, count) at `mu` (0: the 1e-8 the setup leaves): everything the
        solve of `slot` read and wrote, as a dict (lfvio_debug_pass_io).  W is [N, 73] in device landmark order, prior_A [n, n]."""
        N, out, io = n_landmarks, Engine._pass_buffers(n_landmarks), Engine._PassIO()
        Engine._bind_pass(io, out)
        rc = self.lib.lfvio_debug_pass_io(self.ctx, count, slot, float(mu), C.byref(io))
        if rc < 0:
            self._check(rc, "pass_io")
        assert io.num_landmarks == N, (io.num_landmarks, N)
        return Engine._pass_result(io, out, N, rc)

    STATE_DOUBLES = 11 * 7 + 11 * 9 + 7 + 1  # LFVIO_STATE_DOUBLES: pose [11][7] | speed/bias [11][9] | ex [7] | td

    class _StepHeader(C.Structure):  # LfvioStepHeader of include/lfvio_debug.h
        _DOUBLES = ("radius", "mu", "x_cost", "x_norm", "cand_cost", "model_cost_change", "alpha", "grad_sq_total", "gn_sq_total",
                    "grad_gn_total", "gmax_pose", "function_tolerance")
        _INTS = ("iteration", "cur", "do_lin", "do_schur", "done", "termination", "chol_fail", "num_succ", "num_unsucc", "consec_invalid",
                 "trace_len", "skip_step", "spec_n", "max_iter")
        _fields_ = [(k, C.c_double) for k in _DOUBLES] + [("q", C.c_double * 16)] + [(k, C.c_int) for k in _INTS]

        def as_dict(self):
            d = {k: getattr(self, k) for k in self._DOUBLES + self._INTS}
            d["q"] = np.array(self.q[:])
            return d

    class _StepIO(C.Structure):  # LfvioStepIO
        _DOUBLE_ARRAYS = ("scale_l", "diag_l", "grad_l", "einv_l", "lam", "x", "gn_l", "d1", "d2", "step_p", "coef", "cand_x", "cand_lam",
                          "block_sums", "pose_cost")
        _BYTE_ARRAYS = ("cand_tab", "tab_after")

    _StepIO._fields_ = ([("pass_", _PassIO)] + [(k, _dp) for k in _StepIO._DOUBLE_ARRAYS] + [(k, C.POINTER(C.c_ubyte)) for k in _StepIO._BYTE_ARRAYS]
                        + [("x_after", _dp), ("lam_after", _dp), ("trace", C.POINTER(abi.IterationSummary)), ("head", _StepHeader),
                           ("after", _StepHeader)] + [(k, C.c_int) for k in ("head_valid", "num_blocks", "tab_bytes", "spec", "stepw")])

    @staticmethod
    def state_dict(v):
        """A state of LFVIO_STATE_DOUBLES doubles as pose [11, 7], sb [11, 9], ex [7], td."""
        v = np.asarray(v, dtype=np.float64)
        return dict(pose=v[:77].reshape(11, 7).copy(), sb=v[77:176].reshape(11, 9).copy(), ex=v[176:183].copy(), td=float(v[183]))

    def step_io(self, count, slot, n_landmarks, mu=0.0, radius=0.0, spec=1, tabs=False):
        """One whole pass of the resident slots [0, count) at `mu` and `radius` (0: what the setup leaves) with `spec` candidates:
        everything the step half of `slot` read and wrote, as a dict (lfvio_debug_step_io; the first half under the names of
        pass_io).  Landmarks in device order; the per-candidate arrays have `spec` leading entries; head / after are dicts of the
        header's fields, trace the list of the entries this pass pushed.  tabs: the pair tables too (cand_tab [spec, tab_bytes],
        tab_after [tab_bytes] as uint8)."""
        N, KP, SD = n_landmarks, abi.KP, Engine.STATE_DOUBLES
        n1, nb = max(N, 1), max((N + 63) // 64, 1)
        out = Engine._pass_buffers(N)
        io = Engine._StepIO()
        Engine._bind_pass(io.pass_, out)
        more = dict(scale_l=np.zeros(n1), diag_l=np.zeros(n1), grad_l=np.zeros(n1), einv_l=np.zeros(n1), lam=np.zeros(n1), x=np.zeros(SD),
                    gn_l=np.zeros(n1), d1=np.zeros(n1), d2=np.zeros(n1), step_p=np.zeros(KP), coef=np.zeros((4, 5)), cand_x=np.zeros((4, SD)),
                    cand_lam=np.zeros((4, n1)), block_sums=np.zeros((4, nb, 5)), pose_cost=np.zeros((4, 11)), x_after=np.zeros(SD),
                    lam_after=np.zeros(n1))
        for k, a in more.items():
            setattr(io, k, _p(a))
        tab_cap = 32768  # (room for the table: the library reports its size)
        if tabs:
            more.update(cand_tab=np.zeros(4 * tab_cap, np.uint8), tab_after=np.zeros(tab_cap, np.uint8))
            io.cand_tab = more["cand_tab"].ctypes.data_as(C.POINTER(C.c_ubyte))
            io.tab_after = more["tab_after"].ctypes.data_as(C.POINTER(C.c_ubyte))
        trace = (abi.IterationSummary * abi.MAX_TRACE)()
        io.trace = trace
        rc = self.lib.lfvio_debug_step_io(self.ctx, count, slot, float(mu), float(radius), int(spec), C.byref(io))
        if rc < 0:
            self._check(rc, "step_io")
        ps = io.pass_
        assert ps.num_landmarks == N and io.num_blocks == (N + 63) // 64, (ps.num_landmarks, io.num_blocks, N)
        assert 0 < io.tab_bytes <= tab_cap, io.tab_bytes
        Engine._pass_result(ps, out, N, rc)
        for k in ("scale_l", "diag_l", "grad_l", "einv_l", "lam", "gn_l", "d1", "d2", "lam_after"):
            more[k] = more[k][:N]
        more.update(coef=more["coef"][:spec], cand_x=more["cand_x"][:spec], cand_lam=more["cand_lam"][:spec, :N],
                    block_sums=more["block_sums"][:spec, :io.num_blocks], pose_cost=more["pose_cost"][:spec])
        if tabs:
            more.update(cand_tab=more["cand_tab"][:spec * io.tab_bytes].reshape(spec, io.tab_bytes), tab_after=more["tab_after"][:io.tab_bytes])
        out.update(more)
        out.update(head=io.head.as_dict(), after=io.after.as_dict(), head_valid=io.head_valid, num_blocks=io.num_blocks, tab_bytes=io.tab_bytes,
                   spec=io.spec, stepw=io.stepw)
        fields = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_valid",
                  "step_is_successful")
        out["trace"] = [{f: getattr(trace[i], f) for f in fields} for i in range(io.head.trace_len, io.after.trace_len)]
        return out

    def set_function_tolerance(self, tol):
        """Solver::Options::function_tolerance of the windows uploaded from now on (Ceres' default 1e-6)."""
        self.configure("function_tolerance", float(tol))

    def last_chunks(self):
        return int(self.query("last_call", 4)[2])

    def last_passes(self):
        return int(self.query("last_call", 4)[0])

    def force_eig(self, on):
        self.configure("force_eig", int(on))

    def solve(self, win):
        sol = abi.Solution(win.N)
        self._check(self.lib.lfvio_solve(self.ctx, C.byref(win.c()), C.byref(sol.c)), "lfvio_solve")
        return sol

    def solve_relo(self, win, frame, relo_pose, landmark=(), match_point=()):
        """lfvio_solve_relo: the solve with the relocalization factors of one loop-closure message.  Returns
        (abi.Solution, solved relo pose [p, q xyzw])."""
        relo = abi.Relo(frame, relo_pose, landmark, match_point)  # (owns the arrays the ReloC points into: held across the call)
        rc_ = relo.c()
        sol = abi.Solution(win.N)
        out = np.zeros(abi.SIZE_POSE)
        self._check(self.lib.lfvio_solve_relo(self.ctx, C.byref(win.c()), C.byref(rc_), C.byref(sol.c), _p(out)), "lfvio_solve_relo")
        return sol, out

    def solve_relo_rc(self, win, relo, sol, out, num_matches=None, null_arrays=False):
        """The raw return code of lfvio_solve_relo (argument-error tests): outputs are written only on success."""
        rc_ = relo.c(num_matches=num_matches, null_arrays=null_arrays)
        return int(self.lib.lfvio_solve_relo(self.ctx, C.byref(win.c()), C.byref(rc_), C.byref(sol.c), _p(out)))

    def marginalize(self, win, flag):
        prior = abi.Prior()
        self._check(self.lib.lfvio_marginalize(self.ctx, C.byref(win.c()), flag, C.byref(prior)), "lfvio_marginalize")
        return prior

    def schur_repeat(self, win, mu):
        """Largest |difference| between the Schur sums of the mu-retry path and of a full re-linearization (expected 0)."""
        d = np.zeros(1)
        self._check(self.lib.lfvio_debug_schur_repeat(self.ctx, C.byref(win.c()), float(mu), _p(d)), "lfvio_debug_schur_repeat")
        return float(d[0])

    def marg_system(self, n):
        A = np.zeros((n, n))
        b = np.zeros(n)
        self._check(self.lib.lfvio_debug_marg_system(self.ctx, n, _p(A), _p(b)), "lfvio_debug_marg_system")
        return A, b

    def linearize(self, win):
        N = win.N
        H = np.zeros((abi.KP, abi.KP))
        g = np.zeros(abi.KP)
        a, b = np.zeros(max(N, 1)), np.zeros(max(N, 1))
        W = np.zeros((max(N, 1), abi.KC))
        cost = np.zeros(1)
        self._check(self.lib.lfvio_debug_linearize(self.ctx, C.byref(win.c()), _p(H), _p(g), _p(a), _p(b), _p(W),
                                                   _p(cost)), "lfvio_debug_linearize")
        return dict(H=H, g=g, a=a[:N], b=b[:N], W=W[:N], cost=float(cost[0]))

    # ---- device-resident batch API
    def batch_reserve(self, batch, max_landmarks, max_observations):
        self._check(self.lib.lfvio_batch_reserve(self.ctx, batch, max_landmarks, max_observations), "batch_reserve")

    def batch_upload(self, slot, win, marshalled=None):
        """marshalled: the LfvioWindow struct of `win` built beforehand (win.c()); building it is a few hundred Python
        statements — ctypes plumbing of this wrapper, not part of the call a C++ host makes."""
        self._check(self.lib.lfvio_batch_upload(self.ctx, slot, C.byref(marshalled if marshalled is not None else win.c())), "batch_upload")

    def batch_upload_chained(self, slot, win, prior, marshalled=None):
        """The next window of the same estimator: its prior is `prior` (an abi.Prior, in/out) — the one of the call still in
        flight on this context if there is one (collected into `prior` while the window is being packed)."""
        self._check(self.lib.lfvio_batch_upload_chained(self.ctx, slot, C.byref(marshalled if marshalled is not None else win.c()), C.byref(prior)),
                    "batch_upload_chained")

    def set_first_passes(self, n):
        """Debug: > 0 sizes every first graph of the synchronous calls with this many passes (0: from the recent calls again)."""
        self.configure("first_passes", int(n))

    def set_spec_count(self, n):
        """Debug: 1 .. 4 fixes the speculative candidates a pass of a small window prepares (0: from the call before again, 3 or 4).
        The answer is the same bytes for every value (tests/test_spec_candidates.py)."""
        self.configure("spec_count", int(n))

    def last_call(self):
        """(passes the slowest window of the last synchronous call used, iterations they covered, graph launches of that call,
        candidates per pass of the last call that speculated) — lfvio_debug_query "last_call"."""
        return tuple(int(v) for v in self.query("last_call", 4))

    def batch_upload_chained_device(self, slot, win, marshalled=None):
        """The next window of the same estimator, its prior taken over ON THE DEVICE from the call still in flight (no wait, no
        copy of the prior in either direction); win.prior is ignored."""
        self._check(self.lib.lfvio_batch_upload_chained_device(self.ctx, slot, C.byref(marshalled if marshalled is not None else win.c())),
                    "batch_upload_chained_device")

    def batch_optimize(self, count, flag, sync=True):
        fn = self.lib.lfvio_batch_optimize if sync else self.lib.lfvio_batch_optimize_async
        self._check(fn(self.ctx, count, flag), "batch_optimize")

    def batch_sync(self):
        self._check(self.lib.lfvio_batch_sync(self.ctx), "batch_sync")

    def batch_download(self, slot, n_landmarks, want_prior=True, out=None):
        """out: a (Solution, Prior) pair to fill instead of fresh ones (the Prior struct alone is 240 KB to allocate and
        clear: a caller in a loop, like the C++ host side, keeps its output buffers)."""
        sol = out[0] if out is not None else abi.Solution(n_landmarks)
        prior = (out[1] if out is not None else abi.Prior()) if want_prior else None
        self._check(self.lib.lfvio_batch_download(self.ctx, slot, C.byref(sol.c), C.byref(prior) if want_prior else None),
                    "batch_download")
        return sol, prior

    def optimize_begin(self, flag, n_landmarks, out=None):
        """Slot 0: returns the solution as soon as solve + gauge fix are out; the marginalization may still be running."""
        sol = out if out is not None else abi.Solution(n_landmarks)
        self._check(self.lib.lfvio_batch_optimize_begin(self.ctx, flag, C.byref(sol.c)), "batch_optimize_begin")
        return sol

    def optimize_pending(self):
        return bool(self.lib.lfvio_batch_optimize_pending(self.ctx))

    def optimize_finish(self, want_prior=True, out=None):
        prior = (out if out is not None else abi.Prior()) if want_prior else None
        self._check(self.lib.lfvio_batch_optimize_finish(self.ctx, C.byref(prior) if want_prior else None), "batch_optimize_finish")
        return prior

    def optimize(self, win, flag):
        """Whole optimization() of one window on slot 0: solve -> gauge fix -> marginalization."""
        self.batch_reserve(1, win.N, win.M)
        self.batch_upload(0, win)
        self.batch_optimize(1, flag)
        return self.batch_download(0, win.N)

    # ---- SURVEY §8f rank 2
    def triangulate(self, tin, depth):
        """FeatureManager::triangulate on abi.TriangulateIn; returns the updated copy of `depth`."""
        d = np.ascontiguousarray(depth, dtype=np.float64).copy()
        self._check(self.lib.lfvio_triangulate(self.ctx, C.byref(tin.c), _p(d)), "lfvio_triangulate")
        return d

    def shift_depth(self, uv_i, marg_R, marg_P, new_R, new_P, init_depth, depth):
        """Depth arithmetic of FeatureManager::removeBackShiftDepth; returns the updated copy of `depth`."""
        uv = np.ascontiguousarray(uv_i, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(depth, dtype=np.float64).copy()
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (marg_R, marg_P, new_R, new_P)]
        self._check(self.lib.lfvio_shift_depth(self.ctx, len(d), _p(uv), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), float(init_depth), _p(d)),
                    "lfvio_shift_depth")
        return d

    def preintegrate(self, intervals, noise):
        """IntegrationBase over a list of (linearized_ba, linearized_bg, acc_0, gyr_0, dt[], acc[][3], gyr[][3]) intervals
        (the tuple order of synth.Window.raw_imu); returns a list of abi.Preintegration."""
        K = len(intervals)
        arr = (abi.ImuIntervalC * max(K, 1))()
        keep = []
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        for k, (ba, bg, a0, g0, dts, accs, gyrs) in enumerate(intervals):
            dts, accs, gyrs = f(dts).reshape(-1), f(accs).reshape(-1, 3), f(gyrs).reshape(-1, 3)
            keep.append((dts, accs, gyrs))
            arr[k].num_samples = len(dts)
            arr[k].dt, arr[k].acc, arr[k].gyr = _p(dts), _p(accs), _p(gyrs)
            for name, v in (("acc_0", a0), ("gyr_0", g0), ("linearized_ba", ba), ("linearized_bg", bg)):
                setattr(arr[k], name, (C.c_double * 3)(*[float(x) for x in v]))
        out = (abi.Preintegration * max(K, 1))()
        nz = f(noise)
        self._check(self.lib.lfvio_preintegrate(self.ctx, K, arr, _p(nz), out), "lfvio_preintegrate")
        return [out[k] for k in range(K)]

    def two_view(self, bl, br, samples, all_hypotheses=False, out=None, inlier=None, check=True):
        """lfvio_two_view: the two-view RANSAC of ESTIMATE_EXTRINSIC == 2 on bearing pairs bl, br [N, 3] and sample sets
        [S, 8].  Returns the fields of LfvioTwoViewOut as a dict, plus `mask` and, with all_hypotheses, `E_all` [S, 9] and
        `score_all` [S].  out / inlier: a TwoViewOutC / uint8 array to be written (a test of what a failed call leaves
        alone passes its own); check=False returns the error code under `rc` instead of raising."""
        bl = np.ascontiguousarray(bl, dtype=np.float64).reshape(-1, 3)
        br = np.ascontiguousarray(br, dtype=np.float64).reshape(-1, 3)
        sm = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 8)
        tin = abi.TwoViewInC()
        tin.num_matches, tin.num_samples = len(bl), len(sm)
        tin.bearing_l, tin.bearing_r, tin.samples = _p(bl), _p(br), sm.ctypes.data_as(C.POINTER(C.c_int))
        out = abi.TwoViewOutC() if out is None else out
        mask = np.zeros(len(bl), dtype=np.uint8) if inlier is None else inlier
        E_all = np.zeros((len(sm), 9)) if all_hypotheses else None
        score_all = np.zeros(len(sm), dtype=np.float32) if all_hypotheses else None
        rc = self.lib.lfvio_two_view(self.ctx, C.byref(tin), mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out),
                                     _p(E_all) if all_hypotheses else None,
                                     score_all.ctypes.data_as(C.POINTER(C.c_float)) if all_hypotheses else None)
        if check:
            self._check(rc, "lfvio_two_view")
        res = out.as_dict()
        res.update(rc=rc, mask=mask)
        if all_hypotheses:
            res.update(E_all=E_all, score_all=score_all)
        return res

    def vi_align(self, R, T, spans, noise, tic, g_norm, with_pre=False, out=None, x=None, pre=None, check=True):
        """lfvio_vi_align: VisualIMUAlignment on the poses R [F, 3, 3], T [F, 3] of every image of the window and the IMU
        samples between them; spans[k] = (linearized_ba, linearized_bg, acc_0, gyr_0, dt[], acc[][3], gyr[][3]) as for
        preintegrate(), spans[0] is not read (None will do).  Returns the fields of LfvioViAlignOut as a dict plus `x` [3F],
        `rc` and, with with_pre, `pre` (the abi.Preintegration array, entry 0 untouched).  out / x / pre: buffers to be
        written (a test of what a failed call leaves alone passes its own); check=False returns the error code under `rc`
        instead of raising."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        R, T = f(R).reshape(-1, 9), f(T).reshape(-1, 3)
        F = len(spans)
        arr = (abi.ImuIntervalC * max(F, 1))()
        keep = []
        for k, sp in enumerate(spans):
            if k == 0 or sp is None:
                continue
            ba, bg, a0, g0, dts, accs, gyrs = sp
            dts, accs, gyrs = f(dts).reshape(-1), f(accs).reshape(-1, 3), f(gyrs).reshape(-1, 3)
            keep.append((dts, accs, gyrs))
            arr[k].num_samples = len(dts)
            arr[k].dt, arr[k].acc, arr[k].gyr = _p(dts), _p(accs), _p(gyrs)
            for name, v in (("acc_0", a0), ("gyr_0", g0), ("linearized_ba", ba), ("linearized_bg", bg)):
                setattr(arr[k], name, (C.c_double * 3)(*[float(v_) for v_ in v]))
        vin = abi.ViAlignInC()
        vin.num_frames, vin.R, vin.T, vin.span = F, _p(R), _p(T), arr
        vin.noise = (C.c_double * 4)(*[float(v) for v in noise])
        vin.tic = (C.c_double * 3)(*[float(v) for v in tic])
        vin.g_norm = float(g_norm)
        out = abi.ViAlignOutC() if out is None else out
        x = np.zeros(3 * max(F, 1)) if x is None else x
        if pre is None and with_pre:
            pre = (abi.Preintegration * max(F, 1))()
        rc = self.lib.lfvio_vi_align(self.ctx, C.byref(vin), C.byref(out), _p(x), pre)
        if check:
            self._check(rc, "lfvio_vi_align")
        res = out.as_dict()
        res.update(rc=rc, x=x, pre=pre)
        return res

    def pnp(self, offset, point_w, bearing, out=None, check=True):
        """lfvio_pnp: PnpSolver::compute_pose for the F frames of a CSR of correspondences — offset [F + 1], point_w [M, 3] (SfM
        points), bearing [M, 3] (FeaturePerFrame::point as stored).  Returns a list of F dicts with the fields of LfvioPnpOut
        (R [3, 3] and T as compute_pose returns them).  out: an array of abi.PnpOutC to be written (a test of what a failed
        call or a status-1 frame leaves alone passes its own); check=False returns (rc, list) instead of raising."""
        off = np.ascontiguousarray(offset, dtype=np.int32).reshape(-1)
        pw = np.ascontiguousarray(point_w, dtype=np.float64).reshape(-1, 3)
        us = np.ascontiguousarray(bearing, dtype=np.float64).reshape(-1, 3)
        F = len(off) - 1
        pin = abi.PnpInC()
        pin.num_frames, pin.offset, pin.point_w, pin.bearing = F, off.ctypes.data_as(C.POINTER(C.c_int)), _p(pw), _p(us)
        out = (abi.PnpOutC * max(F, 1))() if out is None else out
        rc = self.lib.lfvio_pnp(self.ctx, C.byref(pin), out)
        res = [out[f].as_dict() for f in range(max(F, 0))]
        if check:
            self._check(rc, "lfvio_pnp")
            return res
        return rc, res

    def sfm_ba(self, ref_frame, obs_offset, obs_frame, obs_bearing, c_rotation, c_translation, position, max_num_iterations=-1,
               function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, out=None, check=True):
        """lfvio_sfm_ba: the full BA of GlobalSFM::construct — a CSR over the points' observations (obs_offset [P + 1], obs_frame [M],
        obs_bearing [M, 3]), c_rotation [F, 4] (w x y z), c_translation [F, 3], position [P, 3].  The caller's arrays are not written:
        returns a dict with the fields of LfvioSfmBaOut (Q [F, 4], T [F, 3], trace a list of dicts) plus c_rotation, c_translation,
        position as the call left its own copies, and rc.  out: an abi.SfmBaOutC to be written (a test of what a failed call leaves alone
        passes its own); check=False returns the error code under `rc` instead of raising."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        off, frm = i32(obs_offset), i32(obs_frame)
        us = np.ascontiguousarray(obs_bearing, dtype=np.float64).reshape(-1, 3)
        q, t, X = (np.array(a, dtype=np.float64, order="C").reshape(-1, k) for a, k in ((c_rotation, 4), (c_translation, 3), (position, 3)))
        bin_ = abi.SfmBaInC()
        bin_.num_frames, bin_.ref_frame, bin_.num_points = len(q), int(ref_frame), len(off) - 1
        ip = C.POINTER(C.c_int)
        bin_.obs_offset, bin_.obs_frame, bin_.obs_bearing = off.ctypes.data_as(ip), frm.ctypes.data_as(ip), _p(us)
        bin_.max_num_iterations = int(max_num_iterations)
        bin_.function_tolerance, bin_.gradient_tolerance, bin_.parameter_tolerance = float(function_tolerance), float(gradient_tolerance), float(parameter_tolerance)
        out = abi.SfmBaOutC() if out is None else out
        rc = self.lib.lfvio_sfm_ba(self.ctx, C.byref(bin_), _p(q), _p(t), _p(X), C.byref(out))
        if check:
            self._check(rc, "lfvio_sfm_ba")
        res = out.as_dict(len(q))
        res.update(rc=rc, c_rotation=q, c_translation=t, position=X)
        return res

    def sfm_construct(self, num_frames, ref_frame, obs_offset, obs_frame, obs_bearing, relative_R, relative_T, c_rotation=None, c_translation=None,
                      position=None, tri_op=None, out=None, check=True):
        """lfvio_sfm_construct: the incremental part of GlobalSFM::construct — a CSR over ALL points' observations (obs_offset [P + 1],
        obs_frame [M], obs_bearing [M, 3]) and the relative pose of frames l and F - 1 (relative_R [3, 3], relative_T [3]).  Returns a dict
        with the fields of LfvioSfmConstructOut (pnp a list of F dicts as Engine.pnp returns them) plus c_rotation [F, 4] (w x y z),
        c_translation [F, 3], position [P, 3], tri_op [P] and rc.  The four arrays, and out (an abi.SfmConstructOutC), may be passed in to
        be written (a test of what a failed call or a chain that stops leaves alone passes its own; they are used as they are and must be
        C-contiguous float64 / int32); check=False returns the error code under `rc` instead of raising."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        off, frm = i32(obs_offset), i32(obs_frame)
        us = np.ascontiguousarray(obs_bearing, dtype=np.float64).reshape(-1, 3)
        F, P = int(num_frames), len(off) - 1
        q = np.zeros((max(F, 1), 4)) if c_rotation is None else c_rotation
        t = np.zeros((max(F, 1), 3)) if c_translation is None else c_translation
        X = np.zeros((max(P, 1), 3)) if position is None else position
        ops = np.full(max(P, 1), -1, dtype=np.int32) if tri_op is None else tri_op
        cin = abi.SfmConstructInC()
        cin.num_frames, cin.ref_frame, cin.num_points = F, int(ref_frame), P
        ip = C.POINTER(C.c_int)
        cin.obs_offset, cin.obs_frame, cin.obs_bearing = off.ctypes.data_as(ip), frm.ctypes.data_as(ip), _p(us)
        cin.relative_R = (C.c_double * 9)(*[float(v) for v in np.asarray(relative_R, dtype=np.float64).reshape(-1)])
        cin.relative_T = (C.c_double * 3)(*[float(v) for v in np.asarray(relative_T, dtype=np.float64).reshape(-1)])
        out = abi.SfmConstructOutC() if out is None else out
        rc = self.lib.lfvio_sfm_construct(self.ctx, C.byref(cin), _p(q), _p(t), _p(X), ops.ctypes.data_as(ip), C.byref(out))
        if check:
            self._check(rc, "lfvio_sfm_construct")
        res = out.as_dict(min(max(F, 0), abi.NUM_FRAMES))
        res.update(rc=rc, c_rotation=q[:max(F, 0)], c_translation=t[:max(F, 0)], position=X[:max(P, 0)], tri_op=ops[:max(P, 0)])
        return res

    def relative_pose(self, offsets, bl, br, samples, out=None, inlier=None, check=True):
        """lfvio_relative_pose: Estimator::relativePose over every candidate pair at once — offsets [P + 1] (a CSR over the pairs'
        matches), bl, br [M, 3] and samples [P, S, 8] (indices local to the pair).  Returns a dict with l, relative_R [3, 3],
        relative_T, pair (a list of P dicts with the fields of LfvioRelativePosePair), mask [M] (the refit masks of the pairs that ran)
        and rc.  out / inlier: an abi.RelativePoseOutC / uint8 array to be written (a test of what a failed call leaves alone passes
        its own); check=False returns the error code under `rc` instead of raising."""
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        bl = np.ascontiguousarray(bl, dtype=np.float64).reshape(-1, 3)
        br = np.ascontiguousarray(br, dtype=np.float64).reshape(-1, 3)
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        P = len(off) - 1
        rin = abi.RelativePoseInC()
        rin.num_pairs, rin.num_samples = P, sm.size // (8 * P) if P > 0 else 0
        ip = C.POINTER(C.c_int)
        rin.match_offset, rin.bearing_l, rin.bearing_r, rin.samples = off.ctypes.data_as(ip), _p(bl), _p(br), sm.ctypes.data_as(ip)
        out = abi.RelativePoseOutC() if out is None else out
        mask = np.zeros(max(len(bl), 1), dtype=np.uint8) if inlier is None else inlier
        rc = self.lib.lfvio_relative_pose(self.ctx, C.byref(rin), mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out))
        if check:
            self._check(rc, "lfvio_relative_pose")
        res = out.as_dict(min(max(P, 0), abi.WINDOW_SIZE))
        res.update(rc=rc, mask=mask[:len(bl)])
        return res

    def klt_track(self, image, prev_pts, win_size=41, max_level=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, border=1,
                  next=None, status=None, size=None, num_points=None, want_iterations=True, check=True):
        """lfvio_klt_track: pyramidal Lucas-Kanade of the points prev_pts [N, 2] (float32, in the image of the previous call) into
        `image` [height, width] uint8, which then becomes the resident image.  Returns a dict with next [N, 2] float32, status [N]
        uint8, iterations [N, max_level + 1] (None without want_iterations), levels_used, num_tracked and rc.  next / status: arrays
        to be written, size = (width, height) / num_points: the struct's fields whatever the arrays say, image / prev_pts None: null
        pointers (tests of what a refused call leaves alone); check=False returns the error code under `rc` instead of raising."""
        img = None if image is None else np.ascontiguousarray(image, dtype=np.uint8)
        pts = None if prev_pts is None else np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
        N = (0 if pts is None else len(pts)) if num_points is None else num_points
        kin = abi.KltInC()
        kin.width, kin.height = size if size is not None else (img.shape[1], img.shape[0])
        kin.image = None if img is None else img.ctypes.data_as(C.POINTER(C.c_ubyte))
        kin.num_points = N
        kin.prev_pts = None if pts is None else pts.ctypes.data_as(C.POINTER(C.c_float))
        kin.win_size, kin.max_level, kin.max_iterations, kin.border = win_size, max_level, max_iterations, border
        kin.epsilon, kin.min_eig_threshold = epsilon, min_eig_threshold
        cap = min(max(N, 1), abi.KLT_MAX_POINTS)
        nxt = np.zeros((cap, 2), dtype=np.float32) if next is None else next
        stat = np.zeros(cap, dtype=np.uint8) if status is None else status
        its = np.zeros((cap, min(max(max_level, 0), abi.KLT_MAX_LEVEL) + 1), dtype=np.int32) if want_iterations else None
        out = abi.KltOutC(-1, -1)
        rc = self.lib.lfvio_klt_track(self.ctx, C.byref(kin), nxt.ctypes.data_as(C.POINTER(C.c_float)), stat.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                      its.ctypes.data_as(C.POINTER(C.c_int)) if want_iterations else None, C.byref(out))
        if check:
            self._check(rc, "lfvio_klt_track")
        n = min(max(N, 0), len(stat))
        return dict(next=nxt[:n], status=stat[:n], iterations=its[:n] if want_iterations else None, levels_used=int(out.levels_used),
                    num_tracked=int(out.num_tracked), rc=rc)

    def klt_reset(self):
        """lfvio_klt_reset: forget the resident image; the next klt_track tracks its image against itself."""
        self._check(self.lib.lfvio_klt_reset(self.ctx), "lfvio_klt_reset")

    def klt_level(self, level, check=True):
        """lfvio_klt_level: level `level` of the resident pyramid as a [height, width] uint8 array (None, with check=False, where the
        call is refused: no resident image, or a level no call has built)."""
        w, h = C.c_int(0), C.c_int(0)
        rc = self.lib.lfvio_klt_level(self.ctx, level, C.byref(w), C.byref(h), None)
        if rc != 0 and not check:
            return None
        self._check(rc, "lfvio_klt_level")
        px = np.zeros((h.value, w.value), dtype=np.uint8)
        self._check(self.lib.lfvio_klt_level(self.ctx, level, C.byref(w), C.byref(h), px.ctypes.data_as(C.POINTER(C.c_ubyte))), "lfvio_klt_level")
        return px

    def gft_set_mask(self, mask, size=None, check=True):
        """lfvio_gft_set_mask: the base mask [height, width] uint8 of gft_detect (fisheye_mask, or annulus_mask()); None: all 255
        again.  size = (width, height): the call's fields whatever the array says.  Returns the error code."""
        if mask is None:
            rc = self.lib.lfvio_gft_set_mask(self.ctx, 0, 0, None)
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            w, h = size if size is not None else (m.shape[1], m.shape[0])
            rc = self.lib.lfvio_gft_set_mask(self.ctx, w, h, m.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if check:
            self._check(rc, "lfvio_gft_set_mask")
        return rc

    def gft_detect(self, pts, track_cnt, max_count=150, quality_level=0.01, min_distance=30, mask_radius=30, kept=None, corners=None,
                   num_points=None, check=True):
        """lfvio_gft_detect on the resident image of klt_track: setMask over the tracked points pts [N, 2] float32 with their
        track_cnt [N] int32, then goodFeaturesToTrack for max_count - (number kept) new corners.  Returns a dict with kept (indices
        into pts in kept order), corners [K, 2] float32 in acceptance order, num_candidates, max_response and rc.  kept / corners:
        arrays to be written, num_points: the struct's field whatever the arrays say, pts / track_cnt None: null pointers (tests of
        what a refused call leaves alone); check=False returns the error code under `rc` instead of raising."""
        p = None if pts is None else np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        t = None if track_cnt is None else np.ascontiguousarray(track_cnt, dtype=np.int32).reshape(-1)
        N = (0 if p is None else len(p)) if num_points is None else num_points
        gin = abi.GftInC()
        gin.num_points = N
        gin.pts = None if p is None else p.ctypes.data_as(C.POINTER(C.c_float))
        gin.track_cnt = None if t is None else t.ctypes.data_as(C.POINTER(C.c_int))
        gin.max_count, gin.quality_level, gin.min_distance, gin.mask_radius = max_count, quality_level, min_distance, mask_radius
        kp = np.zeros(min(max(N, 1), abi.KLT_MAX_POINTS), dtype=np.int32) if kept is None else kept
        cr = np.zeros((min(max(max_count, 1), abi.GFT_MAX_CORNERS), 2), dtype=np.float32) if corners is None else corners
        out = abi.GftOutC(-1, -1, -1, -1.0)
        rc = self.lib.lfvio_gft_detect(self.ctx, C.byref(gin), kp.ctypes.data_as(C.POINTER(C.c_int)), cr.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out))
        if check:
            self._check(rc, "lfvio_gft_detect")
        return dict(kept=kp[:max(out.num_kept, 0)], corners=cr[:max(out.num_corners, 0)], num_candidates=int(out.num_candidates),
                    max_response=float(out.max_response), rc=rc)

    def gft_response(self, check=True):
        """lfvio_gft_response: the Shi-Tomasi response lambda of the resident image, [height, width] float64 (None, with check=False,
        where the call is refused: no resident image)."""
        w, h = C.c_int(0), C.c_int(0)
        rc = self.lib.lfvio_klt_level(self.ctx, 0, C.byref(w), C.byref(h), None)
        if rc != 0 and not check:
            return None
        self._check(rc, "lfvio_gft_response")
        out = np.zeros((h.value, w.value), dtype=np.float64)
        self._check(self.lib.lfvio_gft_response(self.ctx, _p(out)), "lfvio_gft_response")
        return out

    def clahe_set(self, clip_limit=3.0, tiles=(8, 8), check=True):
        """lfvio_clahe_set: every later klt_track equalizes its image (CLAHE with `clip_limit` and tiles = (tiles_x, tiles_y)) before
        the pyramid is built, so the resident image is the equalized one; clahe_set(None): off, the state of a fresh context.
        Returns the error code."""
        if clip_limit is None:
            rc = self.lib.lfvio_clahe_set(self.ctx, None)
        else:
            rc = self.lib.lfvio_clahe_set(self.ctx, C.byref(abi.ClaheInC(clip_limit, tiles[0], tiles[1])))
        if check:
            self._check(rc, "lfvio_clahe_set")
        return rc

    def clahe_apply(self, img, clip_limit=3.0, tiles=(8, 8), want_lut=False, out=None, lut=None, size=None, check=True):
        """lfvio_clahe_apply: `img` [height, width] uint8 equalized, as a new array; with want_lut (equalized, lut [tiles_y, tiles_x,
        256] uint8).  Touches neither the resident image nor the setting of clahe_set.  out / lut: arrays to be written, size =
        (width, height): the call's fields whatever the array says, img None: a null pointer (tests of what a refused call leaves
        alone); check=False returns (error code, out, lut) instead."""
        px = None if img is None else np.ascontiguousarray(img, dtype=np.uint8)
        w, h = size if size is not None else (px.shape[1], px.shape[0])
        up = C.POINTER(C.c_ubyte)
        if out is None:
            out = np.zeros((min(max(h, 1), 8192), min(max(w, 1), 8192)), dtype=np.uint8)
        if lut is None and want_lut:
            lut = np.zeros((min(max(tiles[1], 1), abi.CLAHE_MAX_TILES), min(max(tiles[0], 1), abi.CLAHE_MAX_TILES), 256), dtype=np.uint8)
        cin = abi.ClaheInC(clip_limit, tiles[0], tiles[1])
        rc = self.lib.lfvio_clahe_apply(self.ctx, C.byref(cin), w, h, None if px is None else px.ctypes.data_as(up), out.ctypes.data_as(up),
                                        None if lut is None else lut.ctypes.data_as(up))
        if not check:
            return rc, out, lut
        self._check(rc, "lfvio_clahe_apply")
        return (out, lut) if want_lut else out

    def image_format(self, encoding=None, step=0, check=True):
        """lfvio_image_format_set: the images of every later klt_track / track_frame / track_frame_message are `height` rows of `step`
        bytes (0: width * bytes per pixel) in `encoding` (abi.IMG_*), passed as a uint8 array [height, step] with size / width and
        height naming the image's own; image_format(None): off, the state of a fresh context.  Returns the error code."""
        rc = self.lib.lfvio_image_format_set(self.ctx, None if encoding is None else C.byref(abi.ImageFormatC(encoding, step)))
        if check:
            self._check(rc, "lfvio_image_format_set")
        return rc

    def image_gray(self, rows, width, height, encoding=None, step=0, out=None, check=True):
        """lfvio_image_gray: `rows` (uint8, height * step bytes in `encoding`; None: a null pointer) as the grey image [height, width]
        uint8, a new array or `out`.  encoding None: a null format (mono8, rows contiguous).  check=False returns (error code, out)."""
        up = C.POINTER(C.c_ubyte)
        px = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint8)
        if out is None:
            out = np.zeros((min(max(height, 1), 8192), min(max(width, 1), 8192)), dtype=np.uint8)
        rc = self.lib.lfvio_image_gray(self.ctx, None if encoding is None else C.byref(abi.ImageFormatC(encoding, step)), width, height,
                                       None if px is None else px.ctypes.data_as(up), out.ctypes.data_as(up))
        if not check:
            return rc, out
        self._check(rc, "lfvio_image_gray")
        return out

    @staticmethod
    def projector(cam):
        """(ProjectorC or None, keep-alive) from a camera dict (an OCam camera's `inv_poly`: abi.projector_c); None: a null pointer."""
        if cam is None:
            return None, None
        if isinstance(cam, abi.ProjectorC):
            return cam, None
        return abi.projector_c(cam)

    def cam_project(self, cam, P, out=None, n=None, check=True):
        """lfvio_cam_project: spaceToPlane of the points P [n, 3] float64 through `cam` (projector()), as px [n, 2] float64, a new array or
        `out`.  n: the call's field whatever the array says, cam / P None: null pointers (tests of what a refused call leaves alone);
        check=False returns (error code, out)."""
        dp = C.POINTER(C.c_double)
        pts = None if P is None else np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
        n = n if n is not None else len(pts)
        if out is None:
            out = np.zeros((min(max(n, 1), abi.CAM_PROJECT_MAX_POINTS), 2), dtype=np.float64)
        proj, keep = self.projector(cam)
        rc = self.lib.lfvio_cam_project(self.ctx, None if proj is None else C.byref(proj), n, None if pts is None else pts.ctypes.data_as(dp),
                                        out.ctypes.data_as(dp))
        del keep
        if not check:
            return rc, out
        self._check(rc, "lfvio_cam_project")
        return out[:n]

    def remap_build(self, cam, kind, width, height, M=None, want_maps=True, map_x=None, map_y=None, check=True):
        """lfvio_remap_build: the resident map of a width x height output image through `cam` (projector()); kind abi.MAP_EQUIRECT or
        abi.MAP_PERSPECTIVE with M [3, 3] (ray = M (u, v, 1)).  Returns (map_x, map_y) float32 [height, width], or None with
        want_maps=False (both pointers null).  map_x / map_y: arrays to be written, or False: that pointer null whatever want_maps says;
        cam None: a null projector; check=False returns (error code, map_x, map_y)."""
        fp = C.POINTER(C.c_float)
        proj, keep = self.projector(cam)
        m = np.zeros(9) if M is None else np.ascontiguousarray(M, dtype=np.float64).reshape(9)
        rin = abi.RemapInC(None if proj is None else C.pointer(proj), kind, width, height, (C.c_double * 9)(*m.tolist()))
        shape = (min(max(height, 1), 8192), min(max(width, 1), 8192))
        if map_x is None and want_maps:
            map_x = np.zeros(shape, dtype=np.float32)
        if map_y is None and want_maps:
            map_y = np.zeros(shape, dtype=np.float32)
        px = None if map_x is None or map_x is False else map_x.ctypes.data_as(fp)
        py = None if map_y is None or map_y is False else map_y.ctypes.data_as(fp)
        rc = self.lib.lfvio_remap_build(self.ctx, C.byref(rin), px, py)
        del keep
        if not check:
            return rc, map_x, map_y
        self._check(rc, "lfvio_remap_build")
        return (map_x, map_y) if want_maps else None

    def remap_apply(self, rows, src_width, src_height, out_shape, encoding=None, step=0, out=None, check=True):
        """lfvio_remap_apply: `rows` (uint8, src_height * step bytes in `encoding`; None: a null pointer) through the resident map, as
        uint8 [height, width * bytes per pixel] with out_shape = (width, height) of the resident map, a new array or `out`.  encoding
        None: a null format (mono8, rows contiguous).  check=False returns (error code, out)."""
        up = C.POINTER(C.c_ubyte)
        px = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint8)
        if out is None:
            out = np.zeros((out_shape[1], out_shape[0] * abi.IMG_BPP.get(encoding or 0, 4)), dtype=np.uint8)
        rc = self.lib.lfvio_remap_apply(self.ctx, None if encoding is None else C.byref(abi.ImageFormatC(encoding, step)), src_width, src_height,
                                        None if px is None else px.ctypes.data_as(up), out.ctypes.data_as(up))
        if not check:
            return rc, out
        self._check(rc, "lfvio_remap_apply")
        return out

    def remap_reset(self):
        """lfvio_remap_reset: forget the resident map."""
        self._check(self.lib.lfvio_remap_reset(self.ctx), "lfvio_remap_reset")

    def track_source(self, src_width=None, src_height=None, check=True):
        """lfvio_track_source_set: the image of every later klt_track / track_frame / track_frame_message is the SOURCE image —
        src_height rows of src_width pixels in the encoding and step of image_format(), a uint8 array [src_height, step] — and level 0
        is gathered from it through the resident map of remap_build, whose size the calls' size / params width and height must name.
        track_source(None): off, the state of a fresh context.  Returns the error code."""
        rc = self.lib.lfvio_track_source_set(self.ctx, None if src_width is None else C.byref(abi.TrackSourceC(src_width, src_height)))
        if check:
            self._check(rc, "lfvio_track_source_set")
        return rc

    FUSE_OUTPUTS = ("index", "range", "colour", "image_out", "counts")

    def cloud_fuse(self, cloud, n, point_step, offs, width, height, kind=abi.FUSE_EQUIRECT, big_endian=0, R=None, T=None, min_range=0.0,
                   max_range=float("inf"), cam=None, image=None, image_mode=None, encoding=None, step=0, src_size=(0, 0), paint=None,
                   want=("index", "range", "counts"), out=None, check=True):
        """lfvio_cloud_fuse: the n points of `cloud` (uint8, n * point_step bytes: a PointCloud2's data; None: a null pointer) with their
        float32 fields at the byte offsets offs = (off_x, off_y, off_z), through P = R p + T (defaults: the identity) and the range gate,
        onto a width x height image: kind abi.FUSE_EQUIRECT, or abi.FUSE_CAMERA through `cam` (projector()).  image (uint8; None: a null
        pointer): with image_mode abi.FUSE_IMAGE_GIVEN (the default where there is one) the width x height image itself, with
        abi.FUSE_IMAGE_REMAP a src_size = (src_width, src_height) source that goes through the resident map first; encoding None: a null
        format (mono8).  paint: None, or up to four bytes written at every marked pixel.  want: the outputs brought down, of
        FUSE_OUTPUTS; out: {name: array to be written}, taken as they are.  Returns {name: array}; check=False returns (error code, that)."""
        up = C.POINTER(C.c_ubyte)
        data = None if cloud is None else np.ascontiguousarray(cloud, dtype=np.uint8)
        px = None if image is None else np.ascontiguousarray(image, dtype=np.uint8)
        if image_mode is None:
            image_mode = abi.FUSE_IMAGE_NONE if image is None else abi.FUSE_IMAGE_GIVEN
        proj, keep = self.projector(cam)
        fmt = None if encoding is None else abi.ImageFormatC(encoding, step)
        r = np.eye(3).reshape(9) if R is None else np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        t = np.zeros(3) if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(3)
        pb = [int(v) for v in (paint if paint is not None else ())] + [0] * 4
        fin = abi.FuseInC(None if data is None else data.ctypes.data_as(up), n, point_step, offs[0], offs[1], offs[2], big_endian, (C.c_double * 9)(*r.tolist()),
                          (C.c_double * 3)(*t.tolist()), min_range, max_range, kind, width, height, None if proj is None else C.pointer(proj), image_mode,
                          None if fmt is None else C.pointer(fmt), src_size[0], src_size[1], None if px is None else px.ctypes.data_as(up),
                          0 if paint is None else 1, (C.c_ubyte * 4)(*pb[:4]))
        bpp = abi.IMG_BPP.get(encoding or 0, 4)
        nn, w, h = min(max(n, 1), abi.FUSE_MAX_POINTS), min(max(width, 1), 8192), min(max(height, 1), 8192)
        shapes = dict(index=((nn,), np.int32), range=((h, w), np.float32), colour=((nn, bpp), np.uint8), image_out=((h, w * bpp), np.uint8), counts=((3,), np.int32))
        res = dict(out or {})
        for name in want:
            if name not in res:
                res[name] = np.zeros(*shapes[name])
        types = dict(index=C.c_int, range=C.c_float, colour=C.c_ubyte, image_out=C.c_ubyte, counts=C.c_int)
        ptr = {k: res[k].ctypes.data_as(C.POINTER(types[k])) if k in res else None for k in self.FUSE_OUTPUTS}
        fout = abi.FuseOutC(ptr["index"], ptr["range"], ptr["colour"], ptr["image_out"], ptr["counts"])
        rc = self.lib.lfvio_cloud_fuse(self.ctx, C.byref(fin), C.byref(fout))
        del keep
        if not check:
            return rc, res
        self._check(rc, "lfvio_cloud_fuse")
        for name in ("index", "colour"):
            if name in res:
                res[name] = res[name][:n]
        return res

    @staticmethod
    def camera(cam):
        """A CameraC from a dict; None: a null pointer.  model (optional) LFVIO_CAM_OCAM: cx, cy, c, d, e, poly [5];
        LFVIO_CAM_PINHOLE: cx, cy, fx, fy, k1, k2, p1, p2; LFVIO_CAM_MEI: those (u0, v0, gamma1, gamma2 under cx, cy, fx, fy) and xi;
        LFVIO_CAM_KANNALA_BRANDT: cx, cy, fx, fy (u0, v0, mu, mv), k2, k3, k4, k5; LFVIO_CAM_EQUIRECT: fx, fy (abi.camera_c).
        The fields of the other models may be left out (zero)."""
        if cam is None or isinstance(cam, abi.CameraC):
            return cam
        return abi.camera_c(cam)

    def track_reject(self, cam, cur_pts, forw_pts, samples, want_bearings=False, status=None, out=None, bearings=None, num_points=None,
                     num_samples=None, check=True):
        """lfvio_track_reject: rejectWithF on the matches cur_pts -> forw_pts [N, 2] float32 of the camera `cam` (camera()) with the
        sample sets [S, 8].  Returns the fields of LfvioTrackRejectOut as a dict plus mask (= status[], uint8 [N]), rc and, with
        want_bearings, bearing_cur / bearing_forw [N, 3].  status / out / bearings = (cur, forw): buffers to be written, num_points /
        num_samples: the struct's fields whatever the arrays say, cam / cur_pts / forw_pts / samples None: null pointers (tests of
        what a refused call leaves alone); check=False returns the error code under `rc` instead of raising."""
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        cur = None if cur_pts is None else np.ascontiguousarray(cur_pts, dtype=np.float32).reshape(-1, 2)
        forw = None if forw_pts is None else np.ascontiguousarray(forw_pts, dtype=np.float32).reshape(-1, 2)
        sm = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 8)
        N = (0 if cur is None else len(cur)) if num_points is None else num_points
        camc = self.camera(cam)
        rin = abi.TrackRejectInC()
        rin.camera = None if camc is None else C.pointer(camc)
        rin.num_points, rin.num_samples = N, (0 if sm is None else len(sm)) if num_samples is None else num_samples
        rin.cur_pts = None if cur is None else cur.ctypes.data_as(fp)
        rin.forw_pts = None if forw is None else forw.ctypes.data_as(fp)
        rin.samples = None if sm is None else sm.ctypes.data_as(ip)
        cap = min(max(N, 1), abi.TRACK_MAX_POINTS)
        stat = np.zeros(cap, dtype=np.uint8) if status is None else status
        out = abi.TrackRejectOutC() if out is None else out
        bc, bf = bearings if bearings is not None else ((np.zeros((cap, 3)), np.zeros((cap, 3))) if want_bearings else (None, None))
        rc = self.lib.lfvio_track_reject(self.ctx, C.byref(rin), stat.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out),
                                         None if bc is None else _p(bc), None if bf is None else _p(bf))
        if check:
            self._check(rc, "lfvio_track_reject")
        n = min(max(N, 0), len(stat))
        res = dict(status=int(out.status), best_sample=int(out.best_sample), num_inliers=int(out.num_inliers), best_score=float(out.best_score),
                   E=np.array(out.E, dtype=np.float64), mask=stat[:n], rc=rc)
        if bc is not None:
            res.update(bearing_cur=bc[:n], bearing_forw=bf[:n])
        return res

    def track_undistort(self, cam, pts, ids, time, outs=None, num_points=None, want_matched=True, check=True):
        """lfvio_track_undistort: undistortedPoints on cur_pts `pts` [N, 2] float32 with their ids [N] int32 (-1: not yet numbered) at
        cur_time `time`, against the (id, un_pts_3d) pairs the previous call left in the context.  Returns a dict with un_pts [N, 2],
        un_pts_3d [N, 3], velocity_3d [N, 3] (float32), matched [N] int32 (index in the previous call or -1; None without
        want_matched) and rc.  outs = (un_pts, un_pts_3d, velocity_3d, matched): arrays to be written, num_points: the struct's
        field whatever the arrays say, cam / pts / ids None: null pointers; check=False returns the error code under `rc`."""
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        p = None if pts is None else np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        N = (0 if p is None else len(p)) if num_points is None else num_points
        camc = self.camera(cam)
        uin = abi.TrackUndistortInC()
        uin.camera = None if camc is None else C.pointer(camc)
        uin.num_points, uin.time = N, time
        uin.pts = None if p is None else p.ctypes.data_as(fp)
        uin.ids = None if idv is None else idv.ctypes.data_as(ip)
        cap = min(max(N, 1), abi.TRACK_MAX_POINTS)
        if outs is None:
            outs = (np.zeros((cap, 2), np.float32), np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32),
                    np.zeros(cap, np.int32) if want_matched else None)
        un, un3, vel, mt = outs
        rc = self.lib.lfvio_track_undistort(self.ctx, C.byref(uin), un.ctypes.data_as(fp), un3.ctypes.data_as(fp), vel.ctypes.data_as(fp),
                                            None if mt is None else mt.ctypes.data_as(ip))
        if check:
            self._check(rc, "lfvio_track_undistort")
        n = min(max(N, 0), len(un))
        return dict(un_pts=un[:n], un_pts_3d=un3[:n], velocity_3d=vel[:n], matched=None if mt is None else mt[:n], rc=rc)

    def track_reset(self):
        """lfvio_track_reset: forget the resident (id, un_pts_3d) map and time; the next track_undistort gives zero velocities."""
        self._check(self.lib.lfvio_track_reset(self.ctx), "lfvio_track_reset")

    TRACK_FRAME_DEFAULTS = dict(win_size=41, max_level=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, border=1, max_count=150,
                                quality_level=0.01, min_distance=30, mask_radius=30, num_samples=None, capacity=None, width=None, height=None)

    def track_frame(self, img, time, cam, publish=True, words=None, stages=False, out=None, arrays=None, null=(), check=True, _message=None,
                    **params):
        """lfvio_track_frame: `img` [height, width] uint8 at cur_time `time` through readImage on the context's resident track table,
        camera `cam` (camera()), the sample sets drawn on the device from `words` [S, 8] uint32.  params: the fields of
        LfvioTrackFrameIn (TRACK_FRAME_DEFAULTS; num_samples, capacity, width and height default to what the arrays say; capacity to
        4096).  Returns a dict: pts, ids, track_cnt, un_pts, un_pts_3d, velocity_3d (num_points entries each), num_points, num_new,
        levels_used, num_tracked, num_after_reject, reject and detect (dicts of LfvioTrackRejectOut / LfvioGftOut), rc and, with
        stages, stages = dict(next, status, samples (None where none were drawn), mask, kept, corners).  out: a TrackFrameOutC to
        be written; arrays: a dict of the six output arrays; null: names among the six whose pointer is passed as NULL; img / cam /
        words None: null pointers (tests of what a refused call leaves alone); check=False returns the error code under `rc`.
        (_message: track_frame_message's, below.)"""
        unknown = set(params) - set(self.TRACK_FRAME_DEFAULTS)
        if unknown:
            raise TypeError(f"track_frame: unknown parameters {sorted(unknown)}")
        p = dict(self.TRACK_FRAME_DEFAULTS, **params)
        fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
        px = None if img is None else np.ascontiguousarray(img, dtype=np.uint8)
        wd = None if words is None else np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
        camc = self.camera(cam)
        fin = abi.TrackFrameInC()
        fin.width = p["width"] if p["width"] is not None else (0 if px is None else px.shape[1])
        fin.height = p["height"] if p["height"] is not None else (0 if px is None else px.shape[0])
        fin.image = None if px is None else px.ctypes.data_as(up)
        fin.time, fin.publish = time, int(publish)
        fin.camera = None if camc is None else C.pointer(camc)
        for key in ("win_size", "max_level", "max_iterations", "epsilon", "min_eig_threshold", "border", "max_count", "quality_level",
                    "min_distance", "mask_radius"):
            setattr(fin, key, p[key])
        fin.num_samples = p["num_samples"] if p["num_samples"] is not None else (1 if wd is None else len(wd))
        fin.sample_words = None if wd is None else wd.ctypes.data_as(C.POINTER(C.c_uint))
        fin.capacity = abi.TRACK_MAX_POINTS if p["capacity"] is None else p["capacity"]
        cap = abi.TRACK_MAX_POINTS
        if arrays is None:
            arrays = dict(pts=np.zeros((cap, 2), np.float32), ids=np.zeros(cap, np.int32), track_cnt=np.zeros(cap, np.int32),
                          un_pts=np.zeros((cap, 2), np.float32), un_pts_3d=np.zeros((cap, 3), np.float32), velocity_3d=np.zeros((cap, 3), np.float32))
        out = abi.TrackFrameOutC() if out is None else out
        for key, a in arrays.items():
            setattr(out, key, None if key in null else a.ctypes.data_as(ip if a.dtype == np.int32 else fp))
        sg = None
        if stages:
            S = min(max(fin.num_samples, 1), 1024)
            sg = dict(next=np.zeros((cap, 2), np.float32), status=np.zeros(cap, np.uint8), samples=np.zeros((S, 8), np.int32),
                      mask=np.zeros(cap, np.uint8), kept=np.zeros(cap, np.int32), corners=np.zeros((cap, 2), np.float32))
            sc = abi.TrackFrameStagesC(sg["next"].ctypes.data_as(fp), sg["status"].ctypes.data_as(up), sg["samples"].ctypes.data_as(ip),
                                       sg["mask"].ctypes.data_as(up), sg["kept"].ctypes.data_as(ip), sg["corners"].ctypes.data_as(fp))
        before = self.track_frame_count
        if _message is None:
            rc = self.lib.lfvio_track_frame(self.ctx, C.byref(fin), C.byref(out), C.byref(sc) if stages else None)
        else:
            rc = self.lib.lfvio_track_frame_message(self.ctx, C.byref(fin), C.byref(out), C.byref(sc) if stages else None, _message["arg"])
        if check:
            self._check(rc, "lfvio_track_frame" if _message is None else "lfvio_track_frame_message")
        n = min(max(int(out.num_points), 0), cap) if rc == 0 else 0
        res = {key: a[:n] for key, a in arrays.items()}
        rj, dt = out.reject, out.detect
        res.update(num_points=int(out.num_points), num_new=int(out.num_new), levels_used=int(out.levels_used), num_tracked=int(out.num_tracked),
                   num_after_reject=int(out.num_after_reject), rc=rc,
                   reject=dict(status=int(rj.status), best_sample=int(rj.best_sample), num_inliers=int(rj.num_inliers),
                               best_score=float(rj.best_score), E=np.array(rj.E, dtype=np.float64)),
                   detect=dict(num_kept=int(dt.num_kept), num_corners=int(dt.num_corners), num_candidates=int(dt.num_candidates),
                               max_response=float(dt.max_response)))
        if rc == 0:
            self.track_frame_count = n
            if stages:
                n1 = int(out.num_tracked)
                res["stages"] = dict(next=sg["next"][:before], status=sg["status"][:before],
                                     samples=sg["samples"] if publish and n1 >= 8 else None, mask=sg["mask"][:n1] if publish else None,
                                     kept=sg["kept"][:dt.num_kept] if publish else None, corners=sg["corners"][:dt.num_corners] if publish else None)
        return res

    def track_frame_message(self, img, time, cam, rows=None, msg="new", **kw):
        """lfvio_track_frame_message: track_frame's arguments and its dict, plus rows [num_rows, 9] float32 (the node's feature message:
        un_pts_3d, id, pts, velocity_3d of the entries with track_cnt > 1) and num_rows.  rows: the [capacity, 9] float32 array to be
        written (default: a fresh one of 4096 rows); msg: a TrackMessageC to be written, or None for a null pointer; rows=False:
        a null rows pointer (tests of what a refused call leaves alone)."""
        fp = C.POINTER(C.c_float)
        buf = np.zeros((abi.TRACK_MAX_POINTS, 9), np.float32) if rows is None else rows
        m = abi.TrackMessageC() if isinstance(msg, str) else msg
        if m is not None:
            m.rows = None if buf is False else buf.ctypes.data_as(fp)
        res = self.track_frame(img, time, cam, _message=dict(arg=None if m is None else C.byref(m)), **kw)
        n = int(m.num_rows) if (m is not None and res["rc"] == 0) else 0
        res.update(num_rows=n, rows=None if buf is False else buf[:n])
        return res

    def track_frame_reset(self):
        """lfvio_track_frame_reset: klt_reset and track_reset, the track table empty and the next id 0."""
        self._check(self.lib.lfvio_track_frame_reset(self.ctx), "lfvio_track_frame_reset")
        self.track_frame_count = 0

    track_frame_count = 0  # entries of the context's track table, as the last track_frame reported it

    # ---- many streams in one call: the slots of lfvio_track_batch_* (none of them the single route's state)
    def track_batch_reserve(self, slots, check=True):
        """lfvio_track_batch_reserve: `slots` (1 .. 64) empty slots; 0 frees the batch.  Returns the error code."""
        rc = self.lib.lfvio_track_batch_reserve(self.ctx, slots)
        if check:
            self._check(rc, "lfvio_track_batch_reserve")
        if rc == 0:
            self.track_batch_slots = slots
        return rc

    def track_batch_set_mask(self, slot, mask, size=None, check=True):
        """lfvio_track_batch_set_mask: gft_set_mask for slot `slot` (-1: every slot).  Returns the error code."""
        if mask is None:
            rc = self.lib.lfvio_track_batch_set_mask(self.ctx, slot, 0, 0, None)
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            w, h = size if size is not None else (m.shape[1], m.shape[0])
            rc = self.lib.lfvio_track_batch_set_mask(self.ctx, slot, w, h, m.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if check:
            self._check(rc, "lfvio_track_batch_set_mask")
        return rc

    def track_batch_clahe(self, clip_limit=3.0, tiles=(8, 8), check=True):
        """lfvio_track_batch_clahe: clahe_set for the batch; track_batch_clahe(None): off.  Returns the error code."""
        if clip_limit is None:
            rc = self.lib.lfvio_track_batch_clahe(self.ctx, None)
        else:
            rc = self.lib.lfvio_track_batch_clahe(self.ctx, C.byref(abi.ClaheInC(clip_limit, tiles[0], tiles[1])))
        if check:
            self._check(rc, "lfvio_track_batch_clahe")
        return rc

    def track_batch_format(self, encoding=None, step=0, check=True):
        """lfvio_track_batch_format: image_format for the batch; track_batch_format(None): off.  Returns the error code."""
        rc = self.lib.lfvio_track_batch_format(self.ctx, None if encoding is None else C.byref(abi.ImageFormatC(encoding, step)))
        if check:
            self._check(rc, "lfvio_track_batch_format")
        return rc

    def track_batch_reset(self, slot=-1, check=True):
        """lfvio_track_batch_reset: track_frame_reset for slot `slot` (-1: every slot).  Returns the error code."""
        rc = self.lib.lfvio_track_batch_reset(self.ctx, slot)
        if check:
            self._check(rc, "lfvio_track_batch_reset")
        return rc

    def track_batch_map(self, slot, cam=None, kind=None, width=0, height=0, M=None, check=True):
        """lfvio_track_batch_map: remap_build for slot `slot` (-1: every slot, the same recipe in each) — the slot's own resident map
        of a width x height output through `cam` (projector()).  kind None: a null recipe, the slot's map (every map) is forgotten.
        Returns the error code."""
        if kind is None:
            rc = self.lib.lfvio_track_batch_map(self.ctx, slot, None)
        else:
            proj, keep = self.projector(cam)
            m = np.zeros(9) if M is None else np.ascontiguousarray(M, dtype=np.float64).reshape(9)
            rin = abi.RemapInC(None if proj is None else C.pointer(proj), kind, width, height, (C.c_double * 9)(*m.tolist()))
            rc = self.lib.lfvio_track_batch_map(self.ctx, slot, C.byref(rin))
            del keep
        if check:
            self._check(rc, "lfvio_track_batch_map")
        return rc

    def track_batch_source(self, src_width=None, src_height=None, check=True):
        """lfvio_track_batch_source: track_source for the batch — every active image of a later track_batch_frame is the SOURCE image
        (uint8 [src_height, step] in the encoding and step of track_batch_format) and level 0 of slot i is gathered from it through slot
        i's map (track_batch_map), whose size the call's width and height must name.  track_batch_source(None): off.  Returns the
        error code."""
        rc = self.lib.lfvio_track_batch_source(self.ctx, None if src_width is None else C.byref(abi.TrackSourceC(src_width, src_height)))
        if check:
            self._check(rc, "lfvio_track_batch_source")
        return rc

    def track_batch_level(self, slot, level, check=True):
        """lfvio_track_batch_level: klt_level for slot `slot` — level `level` of its resident pyramid as a [height, width] uint8 array
        (None, with check=False, where the call is refused)."""
        w, h = C.c_int(0), C.c_int(0)
        rc = self.lib.lfvio_track_batch_level(self.ctx, slot, level, C.byref(w), C.byref(h), None)
        if rc != 0 and not check:
            return None
        self._check(rc, "lfvio_track_batch_level")
        px = np.zeros((h.value, w.value), dtype=np.uint8)
        self._check(self.lib.lfvio_track_batch_level(self.ctx, slot, level, C.byref(w), C.byref(h), px.ctypes.data_as(C.POINTER(C.c_ubyte))),
                    "lfvio_track_batch_level")
        return px

    def track_batch_frame(self, frames, message=True, count=None, buffers=None, check=True, **params):
        """lfvio_track_batch_frame: frames is a list with one entry per slot — None (the slot is idle in this call) or a dict with img,
        time, cam and, optionally, publish (True), words [S, 8] uint32 and params (fields of LfvioTrackFrameIn for this entry alone).
        **params: the fields every entry shares (Engine.TRACK_FRAME_DEFAULTS).  Returns one dict per slot, shaped like track_frame's
        plus rows [num_rows, 9] and num_rows (None and 0 without `message`); rc is the call's.  count: the call's count whatever the
        list says; buffers: a list of (arrays, TrackFrameOutC, rows) per slot to be written, an array None for a null pointer (tests of
        what a refused call leaves alone); check=False returns the error code under `rc` instead of raising."""
        unknown = set(params) - set(self.TRACK_FRAME_DEFAULTS)
        if unknown:
            raise TypeError(f"track_batch_frame: unknown parameters {sorted(unknown)}")
        fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
        n, cap = len(frames), abi.TRACK_MAX_POINTS
        fin, out, msg = (abi.TrackFrameInC * max(n, 1))(), (abi.TrackFrameOutC * max(n, 1))(), (abi.TrackMessageC * max(n, 1))()
        keep, arrays, rows = [], [], []
        for i, f in enumerate(frames):
            if buffers is not None:
                a, o, r = buffers[i]
                C.memmove(C.byref(out[i]), C.byref(o), C.sizeof(o))
            else:
                a = dict(pts=np.zeros((cap, 2), np.float32), ids=np.zeros(cap, np.int32), track_cnt=np.zeros(cap, np.int32),
                         un_pts=np.zeros((cap, 2), np.float32), un_pts_3d=np.zeros((cap, 3), np.float32), velocity_3d=np.zeros((cap, 3), np.float32))
                r = np.zeros((cap, 9), np.float32)
            arrays.append(a), rows.append(r)
            for key, v in a.items():  # (None: a null pointer)
                setattr(out[i], key, None if v is None else v.ctypes.data_as(ip if v.dtype == np.int32 else fp))
            msg[i].rows = r.ctypes.data_as(fp)
            if buffers is not None:
                msg[i].num_rows = -77
            if f is None:
                continue
            p = dict(self.TRACK_FRAME_DEFAULTS, **params)
            p.update(f.get("params", {}))
            px = None if f.get("img") is None else np.ascontiguousarray(f["img"], dtype=np.uint8)
            wd = None if f.get("words") is None else np.ascontiguousarray(f["words"], dtype=np.uint32).reshape(-1, 8)
            camc = self.camera(f.get("cam"))
            keep.append((px, wd, camc))
            e = fin[i]
            e.width = p["width"] if p["width"] is not None else (0 if px is None else px.shape[1])
            e.height = p["height"] if p["height"] is not None else (0 if px is None else px.shape[0])
            e.image = None if px is None else px.ctypes.data_as(up)
            e.time, e.publish = f["time"], int(f.get("publish", True))
            e.camera = None if camc is None else C.pointer(camc)
            for key in ("win_size", "max_level", "max_iterations", "epsilon", "min_eig_threshold", "border", "max_count", "quality_level",
                        "min_distance", "mask_radius"):
                setattr(e, key, p[key])
            e.num_samples = p["num_samples"] if p["num_samples"] is not None else (1 if wd is None else len(wd))
            e.sample_words = None if wd is None else wd.ctypes.data_as(C.POINTER(C.c_uint))
            e.capacity = cap if p["capacity"] is None else p["capacity"]
        rc = self.lib.lfvio_track_batch_frame(self.ctx, n if count is None else count, fin, out, msg if message else None)
        if check:
            self._check(rc, "lfvio_track_batch_frame")
        res = []
        for i in range(n):
            o = out[i]
            if buffers is not None:
                C.memmove(C.byref(buffers[i][1]), C.byref(o), C.sizeof(o))
            k = min(max(int(o.num_points), 0), cap) if rc == 0 else 0
            r = {key: None if v is None else v[:k] for key, v in arrays[i].items()}
            rj, dt = o.reject, o.detect
            r.update(num_points=int(o.num_points), num_new=int(o.num_new), levels_used=int(o.levels_used), num_tracked=int(o.num_tracked),
                     num_after_reject=int(o.num_after_reject), rc=rc,
                     reject=dict(status=int(rj.status), best_sample=int(rj.best_sample), num_inliers=int(rj.num_inliers),
                                 best_score=float(rj.best_score), E=np.array(rj.E, dtype=np.float64)),
                     detect=dict(num_kept=int(dt.num_kept), num_corners=int(dt.num_corners), num_candidates=int(dt.num_candidates),
                                 max_response=float(dt.max_response)))
            m = int(msg[i].num_rows) if (message and rc == 0) else 0
            r.update(num_rows=m, rows=rows[i][:m] if message else None)
            if buffers is not None:
                r["msg_num_rows"] = int(msg[i].num_rows)
            res.append(r)
        return res

    track_batch_slots = 0  # as the last track_batch_reserve left it

    def time_kernel(self, which, count, reps):
        ms = np.zeros(1)
        self._check(self.lib.lfvio_debug_time_kernel(self.ctx, which, count, reps, _p(ms)), "time_kernel")
        return float(ms[0])

    def sweep_kernel(self, count):
        """Which kernel linearizes a launch over the resident slots [0, count): 0 k_lin (+ k_sum), 1 k_linw, 2 k_linb (+ k_sumb)."""
        return int(self.query("sweep_kernel", 1, float(count))[0])

    def sweep_route(self, count):
        """(the kernel as sweep_kernel gives it, whether k_lin goes out role by role) for a launch over `count` resident slots"""
        q = self.query("sweep_kernel", 2, float(count))
        return int(q[0]), bool(q[1])

    # ---- landmark-sharded API (multi-GPU)
    def shard_begin(self, win, lm_begin, lm_end, add_pose_side):
        self._shard_win = win  # keep the arrays alive
        self._check(self.lib.lfvio_shard_begin(self.ctx, C.byref(win.c()), lm_begin, lm_end, int(add_pose_side)), "shard_begin")

    def shard_exchange(self):
        """(device pointer, total length, scalar offset) of the exchange buffer, in doubles."""
        return (self.lib.lfvio_shard_exchange_ptr(self.ctx), self.lib.lfvio_shard_exchange_len(),
                self.lib.lfvio_shard_scalar_offset())

    def shard_phase(self, name):
        rc = getattr(self.lib, "lfvio_shard_" + name)(self.ctx)
        if rc < 0:
            self._check(rc, "shard_" + name)
        return rc

    def shard_decide(self):
        st = C.c_int(0)
        self._check(self.lib.lfvio_shard_decide(self.ctx, C.byref(st)), "shard_decide")
        return st.value

    def shard_restart(self):
        self._check(self.lib.lfvio_shard_restart(self.ctx), "shard_restart")

    def shard_enqueue(self, phase):
        """Enqueue phase 0..3 of one pass on the context's stream; no host synchronisation."""
        self._check(self.lib.lfvio_shard_enqueue(self.ctx, int(phase)), "shard_enqueue")

    def shard_poll(self):
        """State of the oldest decision not yet read (0 linearize next, 1 step rejected, 2 terminated), or None."""
        st = C.c_int(0)
        rc = self.lib.lfvio_shard_poll(self.ctx, C.byref(st))
        if rc < 0:
            self._check(rc, "shard_poll")
        return st.value if rc == 1 else None

    def shard_marginalize_linearize(self, flag):
        rc = self.lib.lfvio_shard_marg_linearize(self.ctx, int(flag))
        if rc < 0:
            self._check(rc, "shard_marg_linearize")
        return rc

    def shard_marginalize_finish(self, flag):
        prior = abi.Prior()
        self._check(self.lib.lfvio_shard_marg_finish(self.ctx, int(flag), C.byref(prior)), "shard_marg_finish")
        return prior

    def shard_finish(self, n_landmarks_total):
        sol = abi.Solution(n_landmarks_total)
        self._check(self.lib.lfvio_shard_finish(self.ctx, C.byref(sol.c)), "shard_finish")
        return sol

    def stream(self):
        return self.lib.lfvio_stream(self.ctx)


class Group:
    """lfvio_group: the multi-GPU entry points of the C-ABI (RCCL called by the library itself; include/lfvio.h).

    Group(mask=0b11)                      one process, the devices of the mask (ncclCommInitAll)
    Group(rank=r, world=n, device=d, unique_id=b)   one process per GPU (ncclCommInitRank); Group.unique_id() on rank 0,
                                          its 128 bytes broadcast by the launcher
    Group(local_shards=k, device=d)       k ranks on one device, device-side sum instead of RCCL (tests)
    """

    def __init__(self, mask=None, rank=None, world=None, device=0, unique_id=None, local_shards=None, lib_path=None):
        self.lib = abi.load_hip_library(lib_path)
        self.g = None
        if local_shards is not None:
            self.g = self.lib.lfvio_group_create_local(int(device), int(local_shards))
        elif rank is not None:
            assert unique_id is not None and len(unique_id) == 128
            self.g = self.lib.lfvio_group_create_rank(int(device), int(rank), int(world), bytes(unique_id))
        else:
            self.g = self.lib.lfvio_group_create(int(mask if mask is not None else 1))
        if not self.g:
            raise RuntimeError("lfvio_group_create failed (no usable HIP device / RCCL): there is no CPU fallback")
        self._win = None

    @staticmethod
    def unique_id(lib_path=None):
        lib = abi.load_hip_library(lib_path)
        buf = C.create_string_buffer(128)
        if lib.lfvio_group_unique_id(buf) != 0:
            raise RuntimeError("lfvio_group_unique_id failed (librccl not loadable)")
        return buf.raw

    def close(self):
        if self.g:
            self.lib.lfvio_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}: {self.lib.lfvio_group_last_error(self.g).decode()}")

    @property
    def world(self):
        return int(self.lib.lfvio_group_size(self.g))

    @property
    def local(self):
        return int(self.lib.lfvio_group_local(self.g))

    @property
    def rank(self):
        return int(self.lib.lfvio_group_rank(self.g))

    def backend(self):
        return self.lib.lfvio_group_backend(self.g).decode()

    def ctx(self, i=0):
        return self.lib.lfvio_group_ctx(self.g, i)

    def upload(self, win):
        self._win = win  # keep the arrays alive
        self._check(self.lib.lfvio_group_upload(self.g, C.byref(win.c())), "lfvio_group_upload")

    def optimize(self, flag):
        self._check(self.lib.lfvio_group_optimize(self.g, -1 if flag is None else int(flag)), "lfvio_group_optimize")

    def configure(self, key, value=1.0):
        """lfvio_debug_configure on every local context of the group."""
        self.lib.lfvio_debug_configure.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        for i in range(self.local):
            rc = self.lib.lfvio_debug_configure(self.ctx(i), key.encode(), float(value))
            assert rc == 0, rc

    def set_initial_radius(self, r):
        self.configure("initial_radius", r)

    def inject_failure(self, local_ctx, pass_=0, phase=0):
        """tests: local context `local_ctx` fails when it enqueues `phase` of pass `pass_` of the next optimize(); local_ctx < 0 clears"""
        self.lib.lfvio_debug_group_inject_failure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        self._check(self.lib.lfvio_debug_group_inject_failure(self.g, int(local_ctx), int(pass_), int(phase)), "inject_failure")

    def download(self, want_prior=True):
        sol = abi.Solution(self._win.N)
        prior = abi.Prior() if want_prior else None
        self._check(self.lib.lfvio_group_download(self.g, C.byref(sol.c), C.byref(prior) if want_prior else None), "lfvio_group_download")
        return sol, prior

    def solve(self, win, flag):
        """The drop-in call: upload + optimization() + download; returns (solution, prior) — prior None when flag is None."""
        self._win = win
        sol = abi.Solution(win.N)
        prior = abi.Prior() if flag is not None else None
        self._check(self.lib.lfvio_group_solve(self.g, C.byref(win.c()), -1 if flag is None else int(flag), C.byref(sol.c),
                                               C.byref(prior) if prior is not None else None), "lfvio_group_solve")
        return sol, prior

    def range(self, rank):
        b, e = C.c_int(0), C.c_int(0)
        self._check(self.lib.lfvio_group_range(self.g, int(rank), C.byref(b), C.byref(e)), "lfvio_group_range")
        return b.value, e.value

    def last_passes(self):
        return int(self.lib.lfvio_group_last_passes(self.g))

    def last_collectives(self):
        return int(self.lib.lfvio_group_last_collectives(self.g))

    def time_kernel(self, which, count, reps, i=0):
        ms = np.zeros(1)
        self.lib.lfvio_debug_time_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        rc = self.lib.lfvio_debug_time_kernel(self.ctx(i), which, count, reps, _p(ms))
        if rc != 0:
            raise RuntimeError(f"time_kernel failed rc={rc}")
        return float(ms[0])

    def sweep_kernel(self, count, i=0):
        self.lib.lfvio_debug_query.argtypes = [C.c_void_p, C.c_char_p, _dp, C.c_int]
        out = np.array([float(count)])
        rc = self.lib.lfvio_debug_query(self.ctx(i), b"sweep_kernel", _p(out), 1)
        if rc < 0:
            raise RuntimeError(f"sweep_kernel failed rc={rc}")
        return int(out[0])

    # independent windows split over the local devices
    def batch_reserve(self, batch, max_landmarks, max_observations):
        self._check(self.lib.lfvio_group_batch_reserve(self.g, batch, max_landmarks, max_observations), "group_batch_reserve")

    def batch_upload(self, slot, win):
        self._check(self.lib.lfvio_group_batch_upload(self.g, slot, C.byref(win.c())), "group_batch_upload")

    def batch_optimize(self, count, flag):
        self._check(self.lib.lfvio_group_batch_optimize(self.g, count, flag), "group_batch_optimize")

    def batch_download(self, slot, n_landmarks, want_prior=True):
        sol = abi.Solution(n_landmarks)
        prior = abi.Prior() if want_prior else None
        self._check(self.lib.lfvio_group_batch_download(self.g, slot, C.byref(sol.c), C.byref(prior) if want_prior else None), "group_batch_download")
        return sol, prior
