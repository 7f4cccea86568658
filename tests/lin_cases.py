"""The windows of tests/test_lin_hp_ref.py (CPU) and tests/test_lin_hp.py (GPU): the smallest shapes that reach each path of the
residual-and-Jacobian sweep.  Built from lfvio.synth seeds and the small constructors below (the style of all_start_zero in
tests/test_linw.py); a case is built once per session and left unchanged.

CASES maps a name to (constructor(oracle) -> abi.Window, class).  The class of a case is decided here, before anything is computed:
  regular   synthetic windows at the sizes where the kernels change path, the switches, the IMU skip
  prior     a prior puts entries of 1e5 and more beside the unit-sized ones
  edge      numerical edges of the visual factor (inverse depths 1e-3 and 50, no baseline, no motion, an exactly zero residual,
            Cauchy weights down to 1e-4) and an IMU factor kept at sum_dt = 10 exactly
  far       the window translated by (5e3, -3e3, 1e2) m: Xw - Pj cancels
  axis      an observation on (0, 0, 1) and one 1e-9 beside it: the tangent base's branch and the cancellation next to it
  offs      quaternions off the unit sphere by 1e-8 (the OFFS instantiation of the sweep)

Two sizes the work was asked to cover do not exist: a prior's width is 6 a + 9 b + t (a <= 12 pose-sized blocks, b <= 11 speed/bias
blocks, t <= 1 for td), which is 1 or 0 modulo 3 with t = 1 or 0 — never 77 or 89.  Their places are taken by the smallest widths
past LIN_PRIOR_N = 76 and SETUP_TILED_MAXN = 88 that do: 78 (poses 0 .. 9, speed/bias 0, 1) and 90 (poses 0 .. 8, speed/bias 0 .. 3), on
a window without frame-0 landmarks (so that the marginalization plans the upload builds keep at most 76 columns).
"""
import numpy as np

from lfvio import abi, synth

import lin_hp as lh
import np_ref


def _opt(oracle):
    return lambda x, f: oracle.optimize(x, f)


def retrack(src, spec):
    """A window with one landmark per (start_frame, track length) of `spec`, cut from the tracks of `src`: a source track that covers
    the frames is taken (in turn), its first observations dropped where it starts earlier — the inverse depth is then that of the point
    in the new anchor frame, from the window's own state."""
    used = {}
    start, off, lam, pts, vel, ctd, uvy = [], [0], [], [], [], [], []
    s_src, k_src = src.start_frame, np.diff(src.obs_offset)
    for (s, k) in spec:
        assert k >= 2 and s + k <= abi.NUM_FRAMES, (s, k)
        cand = np.nonzero((s_src <= s) & (s_src + k_src >= s + k))[0]
        assert len(cand), (s, k)
        l = int(cand[used.get((s, k), 0) % len(cand)])
        used[(s, k)] = used.get((s, k), 0) + 1
        d = s - int(s_src[l])
        o0 = int(src.obs_offset[l])
        sl = slice(o0 + d, o0 + d + k)
        lm = src.inv_depth[l]
        if d:
            f0 = int(s_src[l])
            Xb = np_ref.qrot(np_ref.pose_q(src.ex_pose), src.obs_point[o0] / lm) + src.ex_pose[:3]
            Xw = np_ref.qrot(np_ref.pose_q(src.pose[f0]), Xb) + src.pose[f0, :3]
            Xbj = np_ref.qrot(np_ref.qinv(np_ref.pose_q(src.pose[s])), Xw - src.pose[s, :3])
            Xcj = np_ref.qrot(np_ref.qinv(np_ref.pose_q(src.ex_pose)), Xbj - src.ex_pose[:3])
            lm = np.linalg.norm(src.obs_point[o0 + d]) / np.linalg.norm(Xcj)
        start.append(s), off.append(off[-1] + k), lam.append(lm)
        pts.append(src.obs_point[sl]), vel.append(src.obs_velocity[sl]), ctd.append(src.obs_cur_td[sl]), uvy.append(src.obs_uv_y[sl])
    return src.copy(start_frame=np.array(start, np.int32), obs_offset=np.array(off, np.int32), inv_depth=np.array(lam), obs_point=np.concatenate(pts),
                    obs_velocity=np.concatenate(vel), obs_cur_td=np.concatenate(ctd), obs_uv_y=np.concatenate(uvy))


def short_tracks(seed, n):
    """n landmarks with tracks of 2 and 3 frames over every start frame 0 .. 9 (start 9: two frames)."""
    spec = [(l % 10, 2 if (l % 10 == 9 or (l // 10) % 2) else 3) for l in range(n)]
    return retrack(synth.make_window(seed, 600), spec)


def all_tracks(seed):
    """every track length 2 .. 11 at every start frame 0 .. 9 that fits the window: 55 landmarks"""
    return retrack(synth.make_window(seed, 900), [(s, k) for s in range(10) for k in range(2, abi.NUM_FRAMES - s + 1)])


def pair_chunks(seed):
    """Tracks of two frames only, so that frame pair (i, i + 1) holds exactly the observations asked for: 1, 15, 16, 17, 63, 64 and 65 (the last
    one spans two chunks of the Gram role); every other pair holds none."""
    counts = {0: 1, 1: 15, 2: 16, 3: 17, 4: 63, 5: 64, 6: 65}
    return retrack(synth.make_window(seed, 900), [(s, 2) for s, c in counts.items() for _ in range(c)])


def with_sum_dt(w, f, sum_dt):
    imu = list(w.imu)
    p = abi.preint_from_array(abi.preint_to_array(imu[f]))
    p.sum_dt = sum_dt  # > 10: the factor is skipped (estimator.cpp:720); exactly 10: kept
    imu[f] = p
    return w.copy(imu=imu)


def off_sphere(w, frames=(), scale_ex=None, eps=1e-8):
    w = w.copy()
    for f in frames:
        w.pose[f, 3:] *= 1.0 + eps
    if scale_ex is not None:
        w.ex_pose[3:] *= 1.0 + scale_ex
    return w


def translated(w, t=(5e3, -3e3, 1e2)):
    w = w.copy()
    w.pose[:, :3] += np.asarray(t)
    return w


def with_depths(w):
    w = w.copy()
    w.inv_depth[0], w.inv_depth[1] = 1e-3, 50.0
    return w


def zero_residual(w):
    """Frames 0 and 1 at the origin with the identity rotation, identity extrinsic, td constant, and a first landmark seen in both with the
    same bearing at lambda = 1: every step of the chain is exact in double and in 50 digits, and the residual is exactly 0 (the `sq_norm ==
    0` side of the corrector's branch)."""
    w = retrack(w, [(0, 2)] + [(int(s), int(k)) for s, k in zip(w.start_frame, np.diff(w.obs_offset))][:6]).copy(estimate_td=0)
    w.pose[0] = w.pose[1] = [0, 0, 0, 0, 0, 0, 1]
    w.ex_pose[:] = [0, 0, 0, 0, 0, 0, 1]
    w.obs_point[1] = w.obs_point[0]
    w.inv_depth[0] = 1.0
    return w


def displaced(w):
    """Observations moved off their bearing so that s = |r|^2 reaches 1e4 (Cauchy weights down to 1e-4)."""
    w = w.copy()
    for l, shift in enumerate((0.01, 0.1, 0.5, 0.94)):
        o = int(w.obs_offset[l]) + 1
        p = w.obs_point[o]
        t = np.cross(p, [0.3, -0.5, 0.8])
        q = p * np.cos(shift) + t / np.linalg.norm(t) * np.sin(shift) * np.linalg.norm(p)
        w.obs_point[o] = q.astype(np.float32).astype(np.float64)
    return w


def on_axis(w):
    w = w.copy()
    o = int(w.obs_offset[0]) + 1
    w.obs_point[o] = [0.0, 0.0, 1.0]
    o = int(w.obs_offset[1]) + 1
    w.obs_point[o] = np.array([1e-9, 0.0, 1.0]) / np.linalg.norm([1e-9, 0.0, 1.0])
    return w


def hand_prior(w, pose_frames, sb_frames, seed):
    """A prior with a random full-rank J0 and r0 over the given blocks, x0 near the state (1e-2)."""
    rng = np.random.default_rng([seed, 60013])
    p = abi.Prior()
    blocks = [(0, f) for f in pose_frames] + [(1, f) for f in sb_frames]
    n = sum(np_ref.block_local(k) for k, _ in blocks)
    p.valid, p.m, p.n, p.num_blocks = 1, 15, n, len(blocks)
    idx = 0
    for i, (k, f) in enumerate(blocks):
        p.blocks[i].kind, p.blocks[i].frame, p.block_idx[i] = k, f, idx
        idx += np_ref.block_local(k)
        if k == 0:
            x0 = np_ref.pose_plus(w.pose[f], rng.normal(0, 1e-2, 6))
            p.block_x0[i][:7] = list(x0)
        else:
            p.block_x0[i][:9] = list(w.speed_bias[f] + rng.normal(0, 1e-2, 9))
    J = rng.normal(0, 1.0, (n, n)) * np.exp(rng.uniform(0, np.log(1e3), n))[:, None] + 10.0 * np.eye(n)
    assert np.linalg.matrix_rank(J) == n
    p.linearized_jacobians[:n * n] = list(J.ravel())
    p.linearized_residuals[:n] = list(rng.normal(0, 1.0, n))
    return w.copy(prior=p)


def no_frame0(seed, n):
    w = synth.make_window(seed, 4 * n)
    spec = [(int(s), int(k)) for s, k in zip(w.start_frame, np.diff(w.obs_offset)) if s > 0][:n]
    return retrack(w, spec)


def second_new(oracle, seed, n):
    """The window behind a MARGIN_SECOND_NEW step: its prior, the solved state, frame 9 taking over frame 10 (slideWindow)."""
    w = synth.make_window_with_prior(seed, n, _opt(oracle))[0]
    sol, prior = oracle.optimize(w, abi.MARGIN_SECOND_NEW)
    assert prior.valid == 1
    w2 = abi.apply_solution(w, sol).copy(prior=prior)
    w2.pose[9], w2.speed_bias[9] = w2.pose[10], w2.speed_bias[10]
    return w2


def negated(w, frame):
    w = w.copy()
    w.pose[frame, 3:] *= -1.0  # the same rotation; the prior's dq.w < 0 branch
    return w


mk = synth.make_window
CASES = {
    # ---- landmark-block edges
    "n1": (lambda o: mk(8, 1), "regular"),
    "n7": (lambda o: mk(3, 7), "regular"),
    "n31": (lambda o: mk(1, 31), "regular"),
    "n32": (lambda o: mk(2, 32), "regular"),
    "n33": (lambda o: mk(5, 33), "regular"),
    "n63": (lambda o: mk(4, 63), "regular"),
    "n64": (lambda o: mk(5, 64), "regular"),
    "n65": (lambda o: mk(6, 65), "regular"),
    "n320": (lambda o: short_tracks(9, 320), "regular"),
    "n321": (lambda o: short_tracks(10, 321), "regular"),
    "all_tracks": (lambda o: all_tracks(11), "regular"),
    # ---- frame-pair chunk edges of the Gram role
    "pair_chunks": (lambda o: pair_chunks(12), "regular"),
    # ---- switches
    "no_td": (lambda o: mk(5, 33, estimate_td=0), "regular"),
    "no_ex": (lambda o: mk(5, 33, estimate_extrinsic=0), "regular"),
    "no_td_no_ex": (lambda o: mk(5, 33, estimate_td=0, estimate_extrinsic=0), "regular"),
    "tr": (lambda o: mk(4, 33, tr=0.02), "regular"),
    "ocam_rs": (lambda o: mk(6, 33, camera="ocam", tr=0.02), "regular"),
    # ---- IMU
    "imu_skip": (lambda o: with_sum_dt(mk(7, 7), 4, 10.5), "regular"),
    "imu_keep10": (lambda o: with_sum_dt(mk(7, 7), 4, 10.0), "edge"),
    # ---- priors
    "prior_old": (lambda o: synth.make_window_with_prior(0, 33, _opt(o))[0], "prior"),
    "prior_second_new": (lambda o: second_new(o, 3, 33), "prior"),
    "prior78": (lambda o: hand_prior(no_frame0(2, 20), range(10), (0, 1), 78), "prior"),
    "prior90": (lambda o: hand_prior(no_frame0(2, 20), range(9), (0, 1, 2, 3), 90), "prior"),
    "prior_negated": (lambda o: negated(synth.make_window_with_prior(0, 33, _opt(o))[0], 3), "prior"),
    # ---- quaternions off the unit sphere
    "offs_frame10": (lambda o: off_sphere(mk(1, 33), (10,)), "offs"),
    "offs_fixed_ex": (lambda o: off_sphere(mk(3, 33, estimate_extrinsic=0), (), 1e-8), "offs"),
    "offs_n321": (lambda o: off_sphere(short_tracks(13, 321), (10,)), "offs"),   # the same on the route of a large window
    # ---- numerical edges
    "far": (lambda o: translated(mk(5, 33)), "far"),
    "far2": (lambda o: translated(mk(6, 31), (-4e3, 6e3, 50.0)), "far"),
    "depths": (lambda o: with_depths(mk(5, 33)), "edge"),
    "rotate": (lambda o: mk(4, 33, motion="rotate"), "edge"),
    "static": (lambda o: mk(4, 33, motion="static"), "edge"),
    "zero_residual": (lambda o: zero_residual(mk(3, 40)), "edge"),
    "displaced": (lambda o: displaced(mk(5, 33)), "edge"),
    "on_axis": (lambda o: on_axis(mk(5, 33)), "axis"),
    "on_axis2": (lambda o: on_axis(mk(4, 31)), "axis"),
}
NAMES = list(CASES)
LARGE = ("n321", "offs_n321")  # past SPEC_MAX_LM = 320: no k_linw; "linw" 2 gives k_linb
CLASSES = ("regular", "prior", "edge", "far", "axis", "offs")

_win = {}


def window(oracle, name):
    if name not in _win:
        _win[name] = CASES[name][0](oracle)
    return _win[name]


def case_class(name):
    return CASES[name][1]


def device_order(w):
    """The device's landmark order -> the caller's (csrc/window_pack.h: a stable sort by (start frame, track length))."""
    return np.argsort(w.start_frame.astype(np.int64) * 16 + np.diff(w.obs_offset), kind="stable")


_stm, _rep = {}, {}


def statement(oracle, name):
    """The 50-digit statement of the case: evaluated once per session."""
    if name not in _stm:
        _stm[name] = lh.Statement(window(oracle, name))
    return _stm[name]


def comparator_reports(oracle, name):
    """Every metric of the two double-precision comparators on the case: computed once per session."""
    if name not in _rep:
        w, stm = window(oracle, name), statement(oracle, name)
        _rep[name] = dict(np_ref=lh.full_report(stm, lh.comparator_np(w), lh.sources_np(w)),
                          oracle=lh.full_report(stm, oracle.linearize(w), lh.sources_oracle(oracle, w)))
    return _rep[name]
