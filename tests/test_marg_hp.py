"""Each stage of k_marg_solve (csrc/kernels_marg.h) against a 50-digit reference (tests/marg_hp.py).

check_prior (tests/test_gpu_parity.py) holds A' and J0^T J0 to 1e-6 of max|A'| ~ 1e6: an absolute bar of about 1.  Here the
Schur complement (stage 1) is held to a 50-digit statement of it in units of u ||H||_2, and the factorization (stage 2) is
judged on the computation's OWN A', b' against the 50-digit spectrum of that A' in units of u ||A'||_2 — eigenvalues, the count at the
eps cut, eigen-residuals, the reconstruction (a direction lost to parallel vectors), r0, and the exact properties of the rows.

CPU tests: the oracle's eigen-solver and LAPACK's eigh go through the same checks on the whole case list — that is how the bars
were measured (8 x the worst of the two) and how they stay honest — and seven corruptions show that each check fails when it should.
GPU tests (-m gpu): one marginalization per case, flag and path on the device.
"""
import numpy as np
import pytest

from lfvio import abi, synth

import marg_hp
import marg_ref

OLD, NEW = abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW


def _skip_imu0(w):
    imu = list(w.imu)
    big = abi.preint_from_array(abi.preint_to_array(imu[0]))
    big.sum_dt = 10.5  # > 10: the factor is skipped (estimator.cpp:720, 858)
    imu[0] = big
    return w.copy(imu=imu)


def _imu_only():
    w = synth.make_window(9, 1)
    return w.copy(start_frame=np.zeros(0, np.int32), obs_offset=np.zeros(1, np.int32), inv_depth=np.zeros(0), obs_point=np.zeros((0, 3)),
                  obs_velocity=np.zeros((0, 3)), obs_cur_td=np.zeros(0), obs_uv_y=np.zeros(0))


# name -> (window, [(with prior, flag)], both paths of the dropped block's pseudo-inverse)
_O, _OP, _NP = (False, OLD), (True, OLD), (True, NEW)
CASES = {
    "full": (lambda: synth.make_window(0, 300), [_O, _OP, _NP], True),            # n = 76 / 70: the shape the benchmark times
    "few_frames": (lambda: synth.make_window(3, 7), [_O, _OP], False),            # n = 46: partial register tiles
    "imu_only": (_imu_only, [_O, _OP], False),                                    # n = 15: A' is cancellation noise
    "one_landmark": (lambda: synth.make_window(11, 1), [_O, _OP], False),         # n = 15 without a prior; the k < 3 reflector branch
    "cut_n40": (lambda: _skip_imu0(synth.make_window(9, 40)), [_O], True),        # n = 49, m = 11: no speed/bias 0 in the dropped block
    "cut_n120": (lambda: _skip_imu0(synth.make_window(9, 120)), [_O], True),      # n = 67, m = 25
    "static": (lambda: synth.make_window(4, 64, motion="static"), [_O, _OP, _NP], False),  # eigenvalues crowded around eps
    "rotate": (lambda: synth.make_window(4, 64, motion="rotate"), [_O, _OP, _NP], False),
    "no_td": (lambda: synth.make_window(5, 64, estimate_td=0), [_O], False),      # column map with holes
    "no_ex": (lambda: synth.make_window(5, 64, estimate_extrinsic=0), [_O], False),
    "no_td_no_ex": (lambda: synth.make_window(5, 64, estimate_td=0, estimate_extrinsic=0), [_O], False),
    "ocam_rs": (lambda: synth.make_window(6, 120, camera="ocam", tr=0.02), [_O], False),   # rolling-shutter td column in the kept block
}
VARIANTS = [(name, pr, flag) for name, (_, vs, _) in CASES.items() for pr, flag in vs]
DEVICE_RUNS = [(name, pr, flag, forced) for name, (_, vs, both) in CASES.items() for pr, flag in vs for forced in ((False, True) if both else (False,))]


def _vid(v):
    return "-".join([v[0], "prior" if v[1] else "noprior", "old" if v[2] == OLD else "second_new"] + (["force_eig"] if len(v) > 3 and v[3] else []))


_windows = {}


def post_gauge(oracle, name):
    """(the oracle's post-gauge state of the case's window, the prior of that call): both sides see identical inputs."""
    if name not in _windows:
        w = CASES[name][0]()
        sol, prior = oracle.optimize(w, OLD)
        _windows[name] = (abi.apply_solution(w, sol), prior)
    return _windows[name]


def variant_window(oracle, name, with_prior):
    w2, prior = post_gauge(oracle, name)
    return w2.copy(prior=prior) if with_prior else w2


_refs = {}


def reference(oracle, v):
    """Everything the CPU knows about a variant, computed once: the oracle's prior and A', b'; the 50-digit Schur complement of the
    oracle's linearization; the 50-digit spectrum of the oracle's A'; the reports of the oracle's and of LAPACK's factor."""
    if v not in _refs:
        name, pr, flag = v
        w = variant_window(oracle, name, pr)
        ref, A, b = oracle.marginalize(w, flag, want_Ab=True)
        assert ref.valid == 1 and ref.n > 0
        lin = oracle.linearize(marg_hp.marg_subwindow(w, flag))
        hp = marg_hp.schur_hp(lin, ref.block_list(), flag)
        lam = marg_hp.eigvals_hp(A)
        Jl, rl = marg_hp.lapack_factor(A, b)
        _refs[v] = dict(w=w, prior=ref, A=A, b=b, lin=lin, hp=hp, lam=lam, s1=marg_hp.stage1_report(A, b, hp),
                        oracle=marg_hp.factor_report(A, b, ref.J(), ref.r(), lam_hp=lam),
                        lapack=marg_hp.factor_report(A, b, Jl, rl, lam_hp=lam))
    return _refs[v]


def _line(tag, rep, s1=None):
    s = (f"{tag}: n={rep['n']} |A'|={rep['normA']:.2e} kept={rep['k']} in_band={rep['in_band']} cut_need={rep['cut_need']:.1f} "
         f"ev={rep['ev']:.2f} res={rep['res']:.2f} recon={rep['recon']:.2f} r={rep['r']:.2f} exact={all(rep['exact'].values())}")
    if s1 is not None:
        s += f" | stage1 dA={s1['dA']:.2f} db={s1['db']:.2f}"
    return s


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the references inside every bar; the restatement pinned; the checks fail when they should
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS, ids=_vid)
def test_both_references_are_inside_every_bar(oracle, v):
    """The oracle's prior and a LAPACK eigh factor of the same A' through factor_report, the oracle's A', b' against schur_hp."""
    R = reference(oracle, v)
    print(_line(_vid(v) + " oracle", R["oracle"], R["s1"]) + f" |H|={R['hp']['normH']:.2e}")
    print(_line(_vid(v) + " lapack", R["lapack"]))
    assert marg_hp.failed_checks(R["oracle"], R["s1"]) == []
    assert marg_hp.failed_checks(R["lapack"]) == []


@pytest.mark.parametrize("v", VARIANTS, ids=_vid)
def test_schur_hp_agrees_with_two_statements_of_the_reference_formula(oracle, v):
    """schur_hp against the oracle's dense A' (the whole m x m dropped block eigen-decomposed, as the reference does it) and against
    numpy's structured statement (marg_ref.structured_marg_old; MARGIN_OLD only), within the stage-1 bar."""
    R = reference(oracle, v)
    assert R["prior"].n == R["hp"]["A"].shape[0]
    assert marg_hp.failed_checks(dict(ev=0, res=0, recon=0, r=0, cut_ok=True, exact={}), R["s1"]) == []
    if v[2] == OLD:
        A, b, _, _ = marg_ref.structured_marg_old(R["lin"], R["prior"].block_list())
        s1 = marg_hp.stage1_report(A, b, R["hp"])
        print(_vid(v), "structured numpy:", s1)
        assert s1["dA"] <= marg_hp.BAR_STAGE1_A and s1["db"] <= marg_hp.BAR_STAGE1_B


def test_the_cut_cases_have_a_dropped_block_with_nine_zero_eigenvalues(oracle):
    """IMU interval 0 skipped and no prior: speed/bias 0 takes no part, the 15 x 15 dropped block of the structured statement has nine
    exactly-zero eigenvalues that the eps cut removes (the oracle and the device plan six columns: m = 6 + landmarks)."""
    for name, m, n in (("cut_n40", 11, 49), ("cut_n120", 25, 67)):
        R = reference(oracle, (name, False, OLD))
        assert (R["prior"].m, R["prior"].n) == (m, n)
        lam = R["hp"]["lam_drop"]
        assert len(lam) == 15 and np.all(lam[:9] == 0.0) and np.all(lam[9:] > marg_hp.EPS)


def test_the_empty_case_is_empty(oracle):
    w2, _ = post_gauge_empty(oracle)
    p = oracle.marginalize(w2, OLD)
    assert (p.valid, p.m, p.n, p.num_blocks) == (1, 0, 0, 0)


def post_gauge_empty(oracle):
    w = _skip_imu0(synth.make_window(9, 7))
    sol, prior = oracle.optimize(w, OLD)
    return abi.apply_solution(w, sol), prior


def _corrupt(R, what):
    """One corruption of the oracle's prior of a window; returns (A, b, J, r) for factor_report."""
    A, b, J, r = R["A"].copy(), R["b"].copy(), R["prior"].J(), R["prior"].r()
    n, k = R["oracle"]["n"], R["oracle"]["k"]
    first = n - k
    i = first + k // 2  # a kept row in the middle of the kept spectrum
    if what == "direction":
        # row i takes its neighbour's direction and keeps its norm (r0 follows the row: only the lost direction is wrong)
        S = (J * J).sum(axis=1)
        J[i] = J[i + 1] * np.sqrt(S[i] / S[i + 1])
        r[i] = (J[i] @ b) / S[i]
    elif what == "scale":
        J[i] *= 1.0 + 1e-9
        r[i] /= 1.0 + 1e-9  # (r0_i = v.b' / sqrt(S) follows the row's new norm)
    elif what == "swap":
        J[[i, i + 1]] = J[[i + 1, i]]
        r[[i, i + 1]] = r[[i + 1, i]]
    elif what == "r":
        r[i] *= 1.0 + 1e-10
    elif what == "zero":
        J[0, 3] = 1e-300
    elif what == "count":
        lam = R["lam"]
        band = marg_hp.BAR_EV * marg_hp.U * R["oracle"]["normA"]
        S = (J * J).sum(axis=1)
        j = min(np.flatnonzero(S > marg_hp.EPS + 2 * band))  # the smallest kept row whose eigenvalue is above the band
        assert lam[j] > marg_hp.EPS + band
        # (the rows below it, inside the band, go with it: dropped rows come first)
        J[: j + 1] = 0.0
        r[: j + 1] = 0.0
    return A, b, J, r


@pytest.mark.parametrize("what,caught", [("direction", ["recon", "res"]), ("scale", ["ev", "recon", "res"]), ("swap", ["ascending"]),
                                         ("r", ["r"]), ("zero", ["zero_rows"]), ("count", ["cut_ok"])])
def test_each_corruption_is_caught_by_its_check_and_no_other(oracle, what, caught):
    """From the oracle's prior of the BASELINE window.  (A row scaled by 1 + 1e-9 is wrong by 2e-9 S in its eigenvalue, and `res` and
    `recon` are stated with that same S_i = ||J_i||^2: the three see one and the same error, so `ev` cannot fail alone.)"""
    R = reference(oracle, ("full", False, OLD))
    assert R["oracle"]["k"] >= 8 and R["oracle"]["n"] - R["oracle"]["k"] >= 1
    assert marg_hp.failed_checks(R["oracle"]) == []
    A, b, J, r = _corrupt(R, what)
    rep = marg_hp.factor_report(A, b, J, r, lam_hp=R["lam"])
    print(what, _line("corrupted", rep))
    assert marg_hp.failed_checks(rep) == sorted(caught)


def test_a_wrong_entry_of_the_schur_complement_is_caught_by_stage_1(oracle):
    R = reference(oracle, ("full", False, OLD))
    A = R["A"].copy()
    A[5, 7] += 1e-3 * R["oracle"]["normA"]
    s1 = marg_hp.stage1_report(A, R["b"], R["hp"])
    assert s1["dA"] > marg_hp.BAR_STAGE1_A and s1["db"] <= marg_hp.BAR_STAGE1_B
    b = R["b"].copy()
    b[3] += 1e-3 * np.abs(b).max()
    s1 = marg_hp.stage1_report(R["A"], b, R["hp"])
    assert s1["db"] > marg_hp.BAR_STAGE1_B and s1["dA"] <= marg_hp.BAR_STAGE1_A


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def same_header(p, ref):
    assert (p.valid, p.m, p.n, p.num_blocks) == (ref.valid, ref.m, ref.n, ref.num_blocks)
    assert p.block_list() == ref.block_list()
    for i in range(p.num_blocks):
        assert np.abs(p.x0(i) - ref.x0(i)).max() < 1e-12


_device_hp, _device_A = {}, {}


@pytest.mark.gpu
@pytest.mark.parametrize("run", DEVICE_RUNS, ids=_vid)
def test_device_marginalization_stage_by_stage(eng, oracle, run):
    """Stage 1 on the device's OWN linearization of the marginalization's factors (the frame-0 sweep of the marginalization runs
    k_lin / k_sum on the same slot data as the debug linearization, so only the algebra is under test), stage 2 on the device's own
    A', b'.  With force_eig the dropped block goes through the Jacobi path and meets the same bars; the two paths' A' agree within
    twice the stage-1 bar."""
    v, forced = run[:3], run[3]
    name, pr, flag = v
    w = variant_window(oracle, name, pr)
    ref = oracle.marginalize(w, flag)
    eng.force_eig(forced)
    try:
        p = eng.marginalize(w, flag)
        A, b = eng.marg_system(p.n)
    finally:
        eng.force_eig(False)
    same_header(p, ref)
    if v not in _device_hp:
        _device_hp[v] = marg_hp.schur_hp(eng.linearize(marg_hp.marg_subwindow(w, flag)), p.block_list(), flag)
    hp = _device_hp[v]
    s1 = marg_hp.stage1_report(A, b, hp)
    rep = marg_hp.factor_report(A, b, p.J(), p.r())
    print(_line("DEVICE " + _vid(run), rep, s1) + f" |H|={hp['normH']:.2e}")
    assert marg_hp.failed_checks(rep, s1) == []
    other = _device_A.get((v, not forced))
    _device_A[(v, forced)] = A
    if other is not None:
        d = np.linalg.norm(A - other, 2) / (marg_hp.U * hp["normH"])
        print(f"DEVICE {_vid(v)}: Cholesky against Jacobi path dA = {d:.2f} u|H|")
        assert d <= 2 * marg_hp.BAR_STAGE1_A


@pytest.mark.gpu
def test_device_empty_marginalization(eng, oracle):
    """No prior, IMU interval 0 skipped, no landmark anchored at frame 0: nothing takes part.  The oracle returns a valid prior
    with m = 0, n = 0 and no blocks, and so must the device."""
    w2, _ = post_gauge_empty(oracle)
    ref = oracle.marginalize(w2, OLD)
    assert (ref.valid, ref.m, ref.n, ref.num_blocks) == (1, 0, 0, 0)
    p = eng.marginalize(w2, OLD)
    same_header(p, ref)


@pytest.mark.gpu
def test_device_second_new_passes_the_prior_through(eng, oracle):
    """MARGIN_SECOND_NEW with a prior that does not touch pose 9, and with no prior: no algebra runs, the prior stays bit for bit."""
    w3, p3 = post_gauge(oracle, "few_frames")  # (few frames: this window's prior does not reach pose 9)
    assert (abi.BLOCK_POSE, 9) not in [(k, f) for (k, f, _) in p3.block_list()]
    w4 = w3.copy(prior=p3)
    ref = oracle.marginalize(w4, NEW)
    q = eng.marginalize(w4, NEW)
    same_header(q, ref)
    assert np.array_equal(q.J(), p3.J()) and np.array_equal(q.r(), p3.r())
    assert np.array_equal(q.J(), ref.J()) and np.array_equal(q.r(), ref.r())
    assert eng.marginalize(w3, NEW).valid == oracle.marginalize(w3, NEW).valid == 0


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [1, 0])
def test_the_prior_of_the_whole_call_belongs_to_the_system_the_context_reports(oracle, ahead):
    """optimization() on the BASELINE window with the marginalization run ahead on worker streams and with the serial tail: the
    prior that comes back — from a worker or from the loop's own tail (tests/test_marg_ahead.py holds the two to the same bits) —
    is the factor of the A', b' that lfvio_debug_marg_system reports, to every bar of stage 2."""
    from lfvio.engine import Engine

    w = synth.make_window_with_prior(0, 300, lambda w_, f: oracle.optimize(w_, f))[0]
    eng = Engine(0)
    try:
        eng.marg_ahead(ahead)
        for rep_no in range(2):  # (the first call of a context sizes its graphs; the second is the steady state)
            sol, prior = eng.optimize(w, OLD)
        A, b = eng.marg_system(prior.n)
        rep = marg_hp.factor_report(A, b, prior.J(), prior.r())
        print(_line(f"DEVICE whole call marg_ahead={ahead} (workers delivered {eng.marg_ahead()[1]})", rep))
        assert prior.valid == 1 and marg_hp.failed_checks(rep) == []
    finally:
        eng.close()
