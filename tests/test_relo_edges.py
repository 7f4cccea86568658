"""The relo route (csrc/kernels_relo.h, csrc/relo.inc) at the edges of what it accepts, against tests/relo_ref.py.

test_relo.py holds the route to relo_ref on windows of at most 300 landmarks, at the default trust-region radius (where
only the Gauss-Newton and Cauchy cases of the dogleg occur) and with the default loop controls.  Here:
  * every case of the traditional dogleg, through a small initial radius on both sides;
  * sizes across the route's thresholds: the 64-landmark workgroups of k_relo_eval, the 1024-lane loops of k_relo_solve,
    its LDS table of RELO_MAX_LM = 2048 landmarks, and the refusal above it;
  * where the matches sit: landmark 0, landmark N - 1, the last (partial) workgroup, every eligible landmark, frames 0 and 9;
  * the other input kinds: OCam + rolling shutter, both prior layouts, quaternions off the unit sphere;
  * the loop controls: iteration caps 0 and 1, function_tolerance, an IMU factor dropped for sum_dt > 10, the wall clock;
  * fixed-order reductions: repeated calls and a context reused across sizes give the same bits.
The bars are test_relo.py's: ref_trace_check, check_state(..., 1e-6), the relo pose at 1e-5, 1e-7 against lfvio_solve."""
import os

import numpy as np
import pytest

import relo_ref
from lfvio import abi, synth
from test_gpu_parity import off_sphere
from test_relo import check_state, load_window, ref_trace_check, rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LFVIO_ERR_ARG = -1
OFFSET = ((0.04, -0.02, 0.01), 1.5)  # the old keyframe: 4 cm / 1.5 deg from the window frame (test_relo.relo_for)


def message(w, frame, K, pick=None, seed=0):
    """relo_ref.Relo of synth.relo_message(w, frame, K); pick: indices into its matches (a subset, still ascending)."""
    m = synth.relo_message(w, frame, K, offset=OFFSET, seed=seed)
    lm, mp = m["landmark"], m["match_point"]
    if pick is not None:
        lm, mp = lm[pick], mp[pick]
    return relo_ref.Relo(frame, w.pose[frame].copy(), lm, mp)


def ends_and_every(n_matches, step):
    """The first and the last match and every step-th one in between."""
    return sorted({0, n_matches - 1} | set(range(0, n_matches, step)))


def solve_relo(eng, w, r_, radius=None, function_tolerance=None):
    try:
        if radius is not None:
            eng.set_initial_radius(radius)
        if function_tolerance is not None:
            eng.set_function_tolerance(function_tolerance)
        return eng.solve_relo(w, r_.frame, r_.relo_pose, r_.landmark, r_.match_point)
    finally:
        eng.set_initial_radius(0)  # (<= 0: Ceres' 1e4)
        eng.set_function_tolerance(1e-6)


def against_relo_ref(eng, w, r_, radius=None, function_tolerance=None, cases=None):
    kw = {}
    if radius is not None:
        kw["radius"] = radius
    if function_tolerance is not None:
        kw["function_tolerance"] = function_tolerance
    x, xr, trace, term = relo_ref.solve(w, r_, cases=cases, **kw)
    sol, rp = solve_relo(eng, w, r_, radius, function_tolerance)
    ref_trace_check(sol, trace, term)
    check_state(sol, x, x.lam, 1e-6)
    assert rel(rp, xr) < 1e-5, rel(rp, xr)
    return sol, rp


def same_bits(a, b):
    """Two solutions (abi.Solution, relo pose) with the same bits in every output."""
    (sa, ra), (sb, rb) = a, b
    for k in ("pose", "speed_bias", "ex_pose", "lam"):
        assert np.array_equal(getattr(sa, k), getattr(sb, k)), k
    assert np.array_equal(ra, rb) and np.float64(sa.td).tobytes() == np.float64(sb.td).tobytes()
    for f in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination", "initial_cost", "final_cost"):
        assert getattr(sa.c, f) == getattr(sb.c, f), f
    assert bytes(sa.c.trace) == bytes(sb.c.trace)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every case of the traditional dogleg (dogleg_strategy.cc ComputeTraditionalDoglegStep)
# ---------------------------------------------------------------------------------------------------------------------
def dogleg_window(kind):
    if kind == "prior":
        return load_window(GOLDEN, "window_n24_prior.npz")
    seed, n, kw = kind
    return synth.make_window(seed, n, max_num_iterations=10, **kw)


# (window, relo frame, matches, initial radius): each starts with Cauchy-point steps, reaches the interpolation case as the
# radius grows back, and ends with Gauss-Newton steps (asserted on relo_ref by the CPU test below)
DOGLEG = [
    ((11, 40, {}), 4, 8, 2.0),
    ((11, 40, {}), 4, 8, 60.0),
    ((12, 40, dict(estimate_td=0, estimate_extrinsic=0)), 9, 8, 5.0),
    ((14, 60, dict(estimate_extrinsic=0)), 6, 12, 5.0),
    ("prior", 4, 5, 2.0),
]
DOGLEG_IDS = ["s11-r2", "s11-r60", "s12-notd-noex-r5", "s14-noex-r5", "n24-prior-r2"]


def test_relo_ref_takes_every_dogleg_case_at_the_chosen_radii():
    """The parameters of the dogleg tests are not vacuous: relo_ref's loop takes the Cauchy point and the interpolation
    between it and the Gauss-Newton step at each of them, and the Gauss-Newton step in all but the prior window (whose
    radius never catches up in its eight iterations).  Of the two forms of beta only c > 0 is ever taken: with
    a = -alpha g and b = -(B + mu I)^-1 g in the D-scaled space, c = a.(b - a) >= 0 by Cauchy-Schwarz once mu -> 0, and mu
    is 1e-8 here."""
    seen = set()
    for kind, frame, K, radius in DOGLEG:
        w = dogleg_window(kind)
        r_ = message(w, frame, K)
        assert r_.K == K
        cases = []
        relo_ref.solve(w, r_, radius=radius, cases=cases)
        assert cases[0] == 1 and 3 in cases, (kind, radius, cases)
        assert kind == "prior" or cases[-1] == 0, (kind, radius, cases)
        seen |= set(cases)
    assert seen == {0, 1, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,frame,K,radius", DOGLEG, ids=DOGLEG_IDS)
def test_every_dogleg_case_vs_relo_ref(eng, kind, frame, K, radius):
    w = dogleg_window(kind)
    r_ = message(w, frame, K)
    cases = []
    sol, _ = against_relo_ref(eng, w, r_, radius=radius, cases=cases)
    assert 1 in cases and 3 in cases
    assert min(t["radius"] for t in sol.trace()) <= radius  # (the device's loop did start there)


@pytest.mark.gpu
def test_function_tolerance_vs_relo_ref(eng):
    """function_tolerance = 1e-3 ends the loop (|cost_change| <= tol * cost, CONVERGENCE) in its 19th iteration, in the middle of
    a run of interpolation steps; with Ceres' 1e-6 the same window runs into its 20-iteration cap."""
    w = synth.make_window(21, 48, max_num_iterations=20)
    r_ = message(w, 6, 20)
    cases = []
    sol, _ = against_relo_ref(eng, w, r_, function_tolerance=1e-3, cases=cases)
    assert sol.c.termination == abi.CONVERGENCE and sol.c.num_iterations < 20 and cases.count(3) >= 5


# ---------------------------------------------------------------------------------------------------------------------
# 2. sizes across the route's thresholds, 3. where the matches sit
# ---------------------------------------------------------------------------------------------------------------------
# (seed, N, relo frame, matches: None every eligible landmark / s the ends and every s-th, iteration cap, landmark 0 matched,
# landmark N - 1 matched)
SIZES = [
    (51, 63, 9, None, 5, True, True),     # one partial workgroup of k_relo_eval
    (52, 64, 0, None, 5, False, False),   # one full workgroup; relo frame 0
    (53, 65, 9, 6, 5, True, True),        # landmark N - 1 alone in the last workgroup
    (54, 1025, 9, None, 2, False, True),  # a second trip of k_relo_solve's 1024-lane loops; 600 matches, landmark N - 1 alone in the last workgroup
    (56, 2048, 9, 20, 2, True, True),     # k_relo_solve's whole hinv table
]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,frame,step,iters,first,last", SIZES, ids=[f"n{s[1]}" for s in SIZES])
def test_sizes_and_match_placement_vs_relo_ref(eng, seed, n, frame, step, iters, first, last):
    w = synth.make_window(seed, n, max_num_iterations=iters)
    full = message(w, frame, n)
    r_ = full if step is None else message(w, frame, n, pick=ends_and_every(full.K, step))
    assert (r_.landmark[0] == 0) == first and (r_.landmark[-1] == n - 1) == last, (r_.landmark[:2], r_.landmark[-2:])
    if step is None and frame == 9:  # every eligible landmark in front of the old keyframe: most of the window
        assert r_.K >= 0.55 * n, r_.K
    against_relo_ref(eng, w, r_)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,lam_tol", [(57, 1023, 1e-7), (58, 1024, 1e-7), (54, 1025, 1e-7), (59, 2047, 1.6e-6), (56, 2048, 1e-7)])
def test_sizes_at_zero_matches_equal_lfvio_solve(eng, seed, n, lam_tol):
    """test_relo.py's 1e-7 against lfvio_solve.  The 2047-landmark window is held at ten times its own floor instead: one ulp of
    one bearing (obs_point[0, 0]) moves relo_ref's (np_ref.solve's) inverse depths by 1.59e-7 of their scale there (6e-10 in
    the 2048-landmark one), so two summation orders cannot be asked to agree to 1e-7."""
    from test_gpu_parity import check_trace_summaries

    w = synth.make_window(seed, n)
    ref = eng.solve(w)
    relo_pose = w.pose[4].copy()
    eng.configure("relo_route", 1)
    try:
        sol, rp = eng.solve_relo(w, 4, relo_pose)
    finally:
        eng.configure("relo_route", 0)
    assert np.array_equal(rp, relo_pose)
    assert sol.c.termination == ref.c.termination and sol.c.num_iterations == ref.c.num_iterations
    tr, rt = sol.trace(), ref.trace()
    assert [t["successful"] for t in tr] == [t["successful"] for t in rt]
    check_trace_summaries(tr, rt)
    for k in ("pose", "speed_bias", "ex_pose"):
        assert rel(getattr(sol, k), getattr(ref, k)) < 1e-7, (k, rel(getattr(sol, k), getattr(ref, k)))
    assert rel(sol.lam, ref.lam) < lam_tol, rel(sol.lam, ref.lam)


@pytest.mark.gpu
def test_more_than_2048_landmarks_are_refused(eng):
    w = synth.make_window(60, 2049)
    r_ = message(w, 9, 40)
    assert r_.K == 40
    for relo, force in ((abi.Relo(9, r_.relo_pose, r_.landmark, r_.match_point), 0), (abi.Relo(9, r_.relo_pose), 1)):
        sol = abi.Solution(w.N)
        sol.inv_depth[:] = 7.0
        out = np.full(abi.SIZE_POSE, 3.0)
        before = bytes(sol.c)
        eng.configure("relo_route", force)
        try:
            rc = eng.solve_relo_rc(w, relo, sol, out)
        finally:
            eng.configure("relo_route", 0)
        assert rc == LFVIO_ERR_ARG, rc
        assert "2048" in eng.lib.lfvio_last_error(eng.ctx).decode()
        assert bytes(sol.c) == before and np.all(out == 3.0) and np.all(sol.inv_depth == 7.0)
    # without a match the call is lfvio_solve, which takes the window
    sol, rp = eng.solve_relo(w, 9, r_.relo_pose)
    assert np.array_equal(rp, r_.relo_pose) and np.array_equal(sol.pose, eng.solve(w).pose)


# ---------------------------------------------------------------------------------------------------------------------
# 4. input kinds with matches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,frame,K,iters", [("window_n120_ocam_rs.npz", 5, 20, 4), ("window_n64_prior_second_new.npz", 3, 10, 8),
                                                ("window_n300_prior.npz", 7, 60, 3)])
def test_golden_windows_with_matches_vs_relo_ref(eng, golden_dir, name, frame, K, iters):
    """OCam + rolling shutter (TR = 0.02: the TR / ROW * row terms of both pts), the MARGIN_SECOND_NEW prior layout, and the
    300-landmark prior window, each with matches on its own landmarks."""
    w = load_window(golden_dir, name)
    w = w.copy(max_num_iterations=min(iters, w.max_num_iterations))
    r_ = message(w, frame, K)
    assert r_.K == K
    against_relo_ref(eng, w, r_)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,frames,ex,eps,relo_eps", [(61, 48, (0, 5, 10), -3e-8, 1e-8, 1e-6), (62, 40, (3, 10), 2e-7, 1e-6, -1e-8)])
def test_quaternions_off_the_unit_sphere_vs_relo_ref(eng, seed, n, frames, ex, eps, relo_eps):
    """Frames, extrinsic and relo pose off the unit sphere (a pose-graph message hands its pose over as it stands): the residual
    chain rotates back with Quaternion::inverse(), the Jacobians with transposes, on both sides."""
    w = off_sphere(synth.make_window(seed, n, max_num_iterations=6), frames, ex, eps=eps)
    frame = 5 if 5 in frames else 9
    r_ = message(w, frame, 12)
    r_.relo_pose[3:] *= 1.0 + relo_eps
    assert abs(np.linalg.norm(r_.relo_pose[3:]) - 1.0) > 0.5 * abs(relo_eps)
    against_relo_ref(eng, w, r_)


# ---------------------------------------------------------------------------------------------------------------------
# 5. loop control
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("iters", [0, 1])
def test_iteration_caps_vs_relo_ref(eng, iters):
    w = synth.make_window(11, 40, max_num_iterations=iters)
    sol, _ = against_relo_ref(eng, w, message(w, 4, 8))
    assert sol.c.termination == abi.NO_CONVERGENCE and sol.c.num_iterations == iters + 1


def long_interval(w, f):
    """The window with IMU interval f longer than 10 s: its IMUFactor is not added (estimator.cpp:720)."""
    imu = [abi.preint_from_array(abi.preint_to_array(p)) for p in w.imu]
    imu[f].sum_dt = 10.5
    return w.copy(imu=imu)


@pytest.mark.gpu
def test_imu_interval_over_ten_seconds_is_dropped(eng):
    """Without the IMU factor of interval 3 the window's td rests on the visual factors alone: one ulp of one bearing
    (obs_point[0, 0]) moves relo_ref's own td by 4.4e-7 of itself (pose 3e-10, inverse depths 2e-9), so td is held at ten times
    that, as test_robustness.py holds the oracle's ill-conditioned blocks to their floor; the rest at check_state's 1e-6."""
    from test_gpu_parity import check_trace_summaries

    w0 = synth.make_window(63, 40)
    w = long_interval(w0, 3)
    r_ = message(w, 6, 10)
    x, xr, trace, term = relo_ref.solve(w, r_)
    sol, rp = solve_relo(eng, w, r_)
    ref_trace_check(sol, trace, term)
    check_state(sol, x, x.lam, 1e-6, td_tol=4.4e-6)
    assert rel(rp, xr) < 1e-5, rel(rp, xr)
    # (not vacuous: the factor's cost is gone from the start point)
    kept, _ = eng.solve_relo(w0, r_.frame, r_.relo_pose, r_.landmark, r_.match_point)
    assert sol.c.initial_cost < kept.c.initial_cost
    ref = eng.solve(w)
    eng.configure("relo_route", 1)
    try:
        sol0, _ = eng.solve_relo(w, 6, r_.relo_pose)
    finally:
        eng.configure("relo_route", 0)
    assert sol0.c.termination == ref.c.termination and sol0.c.num_iterations == ref.c.num_iterations
    check_trace_summaries(sol0.trace(), ref.trace())
    for k in ("pose", "speed_bias", "ex_pose", "lam"):
        assert rel(getattr(sol0, k), getattr(ref, k)) < 1e-7, (k, rel(getattr(sol0, k), getattr(ref, k)))


@pytest.mark.gpu
def test_wall_clock_cap_is_the_iteration_cap_it_ended_at(eng):
    """max_solver_time_in_seconds: the host tests the clock between passes (as lfvio_solve does between graph launches), so a
    cap of 1 ns ends the loop after its first pass — NO_CONVERGENCE, a finite state — at the point a call capped at that many
    iterations ends at, bit for bit.  (Ceres tests the clock at the top of every iteration and would stop before iteration 1;
    include/lfvio.h states the between-passes contract for both entry points.)"""
    w = synth.make_window(11, 40, max_num_iterations=10)
    r_ = message(w, 4, 8)
    capped = solve_relo(eng, w.copy(max_solver_time=1e-9), r_)
    sol = capped[0]
    assert sol.c.termination == abi.NO_CONVERGENCE and 2 <= sol.c.num_iterations < 10
    assert np.isfinite(sol.pose).all() and np.isfinite(sol.lam).all() and np.isfinite(capped[1]).all()
    same_bits(capped, solve_relo(eng, w.copy(max_num_iterations=sol.c.num_iterations - 1), r_))


# ---------------------------------------------------------------------------------------------------------------------
# 6. repeat and reuse: the route reduces in a fixed order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeated_calls_are_bit_identical(eng):
    w = synth.make_window(15, 200, max_num_iterations=10)
    r_ = message(w, 4, 60, seed=15)
    same_bits(solve_relo(eng, w, r_), solve_relo(eng, w, r_))


@pytest.mark.gpu
def test_a_context_reused_across_sizes_gives_the_same_bits(eng):
    """relo_grow keeps the larger device and staging buffers: a 65-landmark window solved right after a 2048-landmark one (rows
    of the larger call still in the buffers) and a 2048-landmark one solved after a 65-landmark one (buffers grown in between)
    give the bits of the same windows on a fresh context."""
    from lfvio.engine import Engine

    big_w = synth.make_window(56, 2048, max_num_iterations=3)
    big = message(big_w, 9, 2048, pick=ends_and_every(message(big_w, 9, 2048).K, 20))
    small_w = synth.make_window(53, 65, max_num_iterations=6)
    small = message(small_w, 9, 65, pick=ends_and_every(message(small_w, 9, 65).K, 6))
    a = b = None
    try:
        a = Engine(0)
        big_fresh = solve_relo(a, big_w, big)
        small_after_big = solve_relo(a, small_w, small)
        b = Engine(0)
        small_fresh = solve_relo(b, small_w, small)
        big_after_small = solve_relo(b, big_w, big)
    finally:
        for e in (a, b):
            if e is not None:
                e.close()
    same_bits(small_after_big, small_fresh)
    same_bits(big_after_small, big_fresh)
