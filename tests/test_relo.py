"""Relocalization factors in optimization() (estimator.cpp:777-808): lfvio_solve_relo against tests/relo_ref.py.

CPU part: the numpy statement itself (relo factor Jacobian by central differences; zero matches = np_ref.solve).
GPU part (-m gpu): the relo route of the library (csrc/kernels_relo.h) against lfvio_solve and against relo_ref."""
import numpy as np
import pytest

import np_ref
import relo_ref
from lfvio import abi, synth


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def relo_for(w, frame, K, seed=0, offset=((0.04, -0.02, 0.01), 1.5)):
    m = synth.relo_message(w, frame, K, offset=offset, seed=seed)
    return relo_ref.Relo(frame, w.pose[frame].copy(), m["landmark"], m["match_point"]), m


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_relo_factor_jacobian_by_central_differences():
    w = synth.make_window(3, 24, max_num_iterations=4)
    st = np_ref.St(w)
    r_, m = relo_for(w, 6, 5)
    assert r_.K >= 3
    l, xy = int(r_.landmark[1]), r_.match_point[1]
    relo_pose = np_ref.pose_plus(r_.relo_pose, np.array([0.01, -0.02, 0.03, 0.01, 0.02, -0.01]))
    _, Ji, Jr, Jex, Jl = relo_ref.relo_factor(w, st, l, relo_pose, xy)
    fi = int(w.start_frame[l])
    h = 1e-6

    def resid(st_, rp):
        return relo_ref.relo_factor(w, st_, l, rp, xy)[0]

    def num(block):
        J = np.zeros((2, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            a, b = st.copy(), st.copy()
            ra, rb = relo_pose.copy(), relo_pose.copy()
            if block == "pose":
                a.pose[fi], b.pose[fi] = np_ref.pose_plus(st.pose[fi], d), np_ref.pose_plus(st.pose[fi], -d)
            elif block == "relo":
                ra, rb = np_ref.pose_plus(relo_pose, d), np_ref.pose_plus(relo_pose, -d)
            else:
                a.ex, b.ex = np_ref.pose_plus(st.ex, d), np_ref.pose_plus(st.ex, -d)
            J[:, k] = (resid(a, ra) - resid(b, rb)) / (2 * h)
        return J

    for block, Ja in (("pose", Ji), ("relo", Jr), ("ex", Jex)):
        Jn = num(block)
        assert np.abs(Ja - Jn).max() <= 1e-6 * max(np.abs(Jn).max(), 1.0), (block, Ja, Jn)
    a, b = st.copy(), st.copy()
    a.lam[l] += h
    b.lam[l] -= h
    Jln = (resid(a, relo_pose) - resid(b, relo_pose)) / (2 * h)
    assert np.abs(Jl - Jln).max() <= 1e-6 * max(np.abs(Jln).max(), 1.0)


def test_relo_ref_with_zero_matches_is_the_plain_solve():
    for w in (synth.make_window(5, 32, max_num_iterations=6), synth.make_window(6, 32, estimate_td=0, estimate_extrinsic=0)):
        x, xr, trace, term = relo_ref.solve(w, relo_ref.Relo(3, w.pose[3]))
        x0, trace0, term0 = np_ref.solve(w)
        assert term == term0 and len(trace) == len(trace0)
        assert [t["successful"] for t in trace] == [t["successful"] for t in trace0]
        assert rel(x.pose, x0.pose) == 0.0 and rel(x.lam, x0.lam) == 0.0
        assert np.array_equal(xr, w.pose[3])


def solved_window(w, x):
    return w.copy(pose=x.pose, speed_bias=x.sb, ex_pose=x.ex, td=x.td, inv_depth=x.lam)


def test_relo_ref_recovers_the_old_keyframe():
    """A window started from its own (iteration-capped) solve and matches projected from that state into an old keyframe
    4 cm / 1.5 deg away: the relo pose moves to the old keyframe's pose.  The window is not exactly at a stationary point of
    its own objective (it keeps moving ~1.5 cm in a second solve), which bounds the recovery: 5 mm of the 47 mm offset remain."""
    w0 = synth.make_window(7, 48, max_num_iterations=30)
    x0, _, _ = np_ref.solve(w0)
    w = solved_window(w0, x0)
    r_, m = relo_for(w, 4, 40)
    assert r_.K >= 15
    x, xr, trace, term = relo_ref.solve(w, r_)
    d0 = np.abs(r_.relo_pose[:3] - m["old_pose"][:3]).max()
    d1 = np.abs(xr[:3] - m["old_pose"][:3]).max()
    assert d1 < 0.25 * d0, (d0, d1)


def test_relo_tail_recovers_an_injected_drift():
    """double2vector's relo tail at the exact answer: the drift and the relative pose come back to rounding."""
    w = synth.make_window(8, 24)
    frame = 5
    m = synth.relo_message(w, frame, 10, drift_yaw_deg=7.0, drift_t=(0.3, -0.2, 0.05), offset=((0.0, 0.0, 0.0), 0.0))
    P0 = w.pose[0][:3]
    out = relo_ref.relo_tail(np.eye(3), P0, w.pose[0], m["old_pose"], m["relo_t"], m["relo_r"], w.pose[frame][:3],
                             synth.pose_R(w.pose[frame]))
    assert abs(out["drift_correct_yaw"] - 7.0) < 1e-9
    assert np.abs(out["drift_correct_t"] - np.array([0.3, -0.2, 0.05])).max() < 1e-9
    assert np.abs(out["relo_relative_t"]).max() < 1e-9 and abs(out["relo_relative_yaw"]) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def load_window(golden_dir, name):
    import os

    d = np.load(os.path.join(golden_dir, name))
    return abi.window_from_dict({k[4:]: d[k] for k in d.files if k.startswith("win_")})


def check_state(sol, ref_x, ref_lam, tol, td_tol=None):
    assert rel(sol.pose, ref_x.pose) < tol, rel(sol.pose, ref_x.pose)
    assert rel(sol.speed_bias, ref_x.sb) < tol, rel(sol.speed_bias, ref_x.sb)
    assert rel(sol.ex_pose, ref_x.ex) < tol
    assert abs(sol.td - ref_x.td) <= (td_tol or tol) * max(abs(ref_x.td), 1e-300), (sol.td, ref_x.td)
    assert rel(sol.lam, ref_lam) < tol, rel(sol.lam, ref_lam)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window_n24.npz", "window_n24_notd_noex.npz", "window_n24_rs.npz", "window_n24_prior.npz",
                                  "window_n300_prior.npz"])
def test_route_at_zero_matches_equals_lfvio_solve(eng, golden_dir, name):
    from test_gpu_parity import check_trace_summaries

    w = load_window(golden_dir, name)
    ref = eng.solve(w)
    relo_pose = w.pose[4].copy()
    relo_pose[0] += 0.25
    eng.configure("relo_route", 1)
    try:
        sol, rp = eng.solve_relo(w, 4, relo_pose)
    finally:
        eng.configure("relo_route", 0)
    assert np.array_equal(rp, relo_pose)
    assert sol.c.termination == ref.c.termination and sol.c.num_iterations == ref.c.num_iterations
    tr, rt = sol.trace(), ref.trace()
    assert [t["successful"] for t in tr] == [t["successful"] for t in rt]
    assert [t["valid"] for t in tr] == [t["valid"] for t in rt]
    check_trace_summaries(tr, rt)
    # (the same arithmetic summed in another order: k_relo_gram / k_relo_schur against k_lin / k_sum / k_solve_dense; over an
    # iteration-capped solve the rounding grows to ~1e-8 of the state, measured worst 9e-9)
    for k in ("pose", "speed_bias", "ex_pose", "lam"):
        assert rel(getattr(sol, k), getattr(ref, k)) < 1e-7, (k, rel(getattr(sol, k), getattr(ref, k)))
    # the delegating path (no debug key) copies the pose through as well
    sol2, rp2 = eng.solve_relo(w, 4, relo_pose)
    assert np.array_equal(rp2, relo_pose) and np.array_equal(sol2.pose, ref.pose)


CASES = [
    # (seed, N, kw, frame, K)
    (11, 40, {}, 4, 1),
    (12, 40, dict(estimate_td=0, estimate_extrinsic=0), 9, 2),
    (13, 120, dict(estimate_td=0), 0, 5),
    (14, 200, dict(estimate_extrinsic=0), 9, 60),
    (15, 200, {}, 4, 60),
    (16, 300, {}, 9, 60),
]


def ref_trace_check(sol, trace, term):
    """Same decisions, same trace to rounding.  relo_ref solves the full (172 + N + 6) system by a dense Cholesky, the route
    through the Schur complement of the landmark block: the two differ by rounding that an iteration-capped solve carries
    into a rejected step's candidate cost (measured 5e-6 of one cost_change of 0.1 at a cost of 47), so the trace is held at
    1e-5 relative here rather than at check_trace_summaries' 1e-6."""
    tr = sol.trace()
    assert sol.c.termination == term, (sol.c.termination, term)
    assert len(tr) == len(trace), (len(tr), len(trace))
    assert [t["successful"] for t in tr] == [t["successful"] for t in trace]
    assert [t["valid"] for t in tr] == [t["valid"] for t in trace]
    assert rel([t["radius"] for t in tr], [t["radius"] for t in trace]) < 1e-6
    assert rel([t["cost"] for t in tr], [t["cost"] for t in trace]) < 1e-7
    for k, (a, b) in enumerate(zip(tr, trace)):
        for f in ("gradient_max_norm", "step_norm", "cost_change", "relative_decrease"):
            if np.isnan(b[f]):
                assert np.isnan(a[f]), (k, f)
                continue
            assert abs(a[f] - b[f]) <= 1e-5 * abs(b[f]) + 1e-9 * abs(b["cost"]), (k, f, a[f], b[f])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,kw,frame,K", CASES)
def test_route_vs_relo_ref(eng, seed, n, kw, frame, K):
    w = synth.make_window(seed, n, max_num_iterations=10, **kw)
    r_, _ = relo_for(w, frame, K, seed=seed)
    assert r_.K == K, (r_.K, K)
    x, xr, trace, term = relo_ref.solve(w, r_)
    sol, rp = eng.solve_relo(w, frame, r_.relo_pose, r_.landmark, r_.match_point)
    ref_trace_check(sol, trace, term)
    check_state(sol, x, x.lam, 1e-6)
    # (the relo pose rests on the K relocalization factors alone and is the worst-conditioned block: measured 1.4e-6)
    assert rel(rp, xr) < 1e-5, rel(rp, xr)


@pytest.mark.gpu
def test_route_vs_relo_ref_with_prior(eng, golden_dir):
    w = load_window(golden_dir, "window_n24_prior.npz")
    r_, _ = relo_for(w, 4, 5)
    assert r_.K == 5
    x, xr, trace, term = relo_ref.solve(w, r_)
    sol, rp = eng.solve_relo(w, 4, r_.relo_pose, r_.landmark, r_.match_point)
    ref_trace_check(sol, trace, term)
    check_state(sol, x, x.lam, 1e-6)
    assert rel(rp, xr) < 1e-5


@pytest.mark.gpu
def test_kkt_at_a_converged_relo_solution(eng):
    w = synth.make_window(21, 48, max_num_iterations=50)
    r_, _ = relo_for(w, 6, 20)
    sol, rp = eng.solve_relo(w, 6, r_.relo_pose, r_.landmark, r_.match_point)
    assert sol.c.termination == abi.CONVERGENCE
    st0 = np_ref.St(w)
    g0 = relo_ref.objective_gradient(w, st0, r_, r_.relo_pose)
    st = np_ref.St(abi.apply_solution(w, sol))
    g = relo_ref.objective_gradient(w, st, r_, rp)
    assert np.abs(g).max() < 1e-3 * np.abs(g0).max(), (np.abs(g).max(), np.abs(g0).max())


@pytest.mark.gpu
def test_malformed_relo_is_refused_and_outputs_untouched(eng):
    w = synth.make_window(31, 24)
    r_, _ = relo_for(w, 6, 4)
    assert r_.K == 4
    late = int(np.argmax(w.start_frame > 2))
    assert w.start_frame[late] > 2
    cases = [
        (abi.Relo(-1, r_.relo_pose, r_.landmark, r_.match_point), {}),
        (abi.Relo(abi.WINDOW_SIZE, r_.relo_pose, r_.landmark, r_.match_point), {}),
        (abi.Relo(6, r_.relo_pose, [0, w.N], [[0.1, 0.1], [0.2, 0.2]]), {}),
        (abi.Relo(6, r_.relo_pose, [-1], [[0.1, 0.1]]), {}),
        (abi.Relo(6, r_.relo_pose, r_.landmark[::-1].copy(), r_.match_point), {}),
        (abi.Relo(6, r_.relo_pose, [r_.landmark[0], r_.landmark[0]], [[0.1, 0.1], [0.2, 0.2]]), {}),
        (abi.Relo(2, r_.relo_pose, [late], [[0.1, 0.1]]), {}),
        (abi.Relo(6, r_.relo_pose, r_.landmark, r_.match_point), dict(num_matches=-1)),
        (abi.Relo(6, r_.relo_pose, r_.landmark, r_.match_point), dict(null_arrays=True)),
    ]
    for relo, kw in cases:
        sol = abi.Solution(w.N)
        sol.inv_depth[:] = 7.0
        out = np.full(abi.SIZE_POSE, 3.0)
        before = bytes(sol.c)
        assert eng.solve_relo_rc(w, relo, sol, out, **kw) == -1, (relo.frame, relo.landmark, kw)
        assert bytes(sol.c) == before and np.all(out == 3.0) and np.all(sol.inv_depth == 7.0)


@pytest.mark.gpu
def test_known_answer_drift_through_the_relo_tail(eng):
    """A window at its own solution, a loop to an old keyframe 4 cm / 1.5 deg away whose pose-graph pose carries an injected drift
    (12 deg yaw, 0.5 m): solve, then double2vector's relo tail (gauge fix with the reference's rot_diff) recovers the drift.
    The matches are exact (no pixel noise); what bounds the recovery is how far the window itself still moves in the solve
    (the synthetic window is re-solved with the loop's factors and settles elsewhere by a few millimetres; measured 0.17 deg
    of drift yaw): 0.5 deg of yaw, 5 cm of translation."""
    w0 = synth.make_window(41, 120, max_num_iterations=20)
    w = solved_window(w0, np_ref.St(abi.apply_solution(w0, eng.solve(w0))))
    frame = 7
    m = synth.relo_message(w, frame, 60, drift_yaw_deg=12.0, drift_t=(0.5, -0.3, 0.1), offset=((0.04, -0.02, 0.01), 1.5))
    sol, rp = eng.solve_relo(w, frame, w.pose[frame], m["landmark"], m["match_point"])
    st = np_ref.gauge_fix(w.pose[0], np_ref.St(abi.apply_solution(w, sol)))
    # rot_diff / origin_P0 of double2vector (no pitch singularity here): yaw of the start pose minus yaw of the solved one
    Rs0 = synth.pose_R(w.pose[0])
    R00 = synth.pose_R(sol.pose[0])
    rot_diff = relo_ref.ypr2R([relo_ref.R2ypr(Rs0)[0] - relo_ref.R2ypr(R00)[0], 0, 0])
    out = relo_ref.relo_tail(rot_diff, w.pose[0][:3], sol.pose[0], rp, m["relo_t"], m["relo_r"], st.pose[frame][:3],
                             synth.pose_R(st.pose[frame]))
    assert abs(out["drift_correct_yaw"] - 12.0) < 0.5, out["drift_correct_yaw"]
    assert np.abs(out["drift_correct_t"] - np.array([0.5, -0.3, 0.1])).max() < 0.05, out["drift_correct_t"]
    # relative pose of the window frame to the old keyframe: the offset that was put between them
    R_old = synth.pose_R(m["old_pose"])
    exp_t = R_old.T @ (w.pose[frame][:3] - m["old_pose"][:3])
    assert np.abs(out["relo_relative_t"] - exp_t).max() < 0.05
    assert abs(out["relo_relative_yaw"] - (-1.5)) < 0.5, out["relo_relative_yaw"]
