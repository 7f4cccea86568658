"""lfvio_sfm_ba (k_sfm_ba) against a 50-digit reference and against the numpy restatement (tests/sfm_ba_ref.py).

The fixtures tests/golden/sfm_ba_hp.npz hold one bundle-adjustment case per regime and, from the 50-digit side, the cost, gradient and
reduced camera system at the start and the minimiser of the gauge-fixed problem; tests/golden/gen_sfm_ba_hp.py writes them and lists
the regimes.  Metrics, in units of eps = 2^-52:

  cost0   |initial_cost - 50-digit cost| / cost                      gmax0  the same for iteration 0's gradient_max_norm
  R, RQ   largest |difference| of an entry of the rotation matrices of c_rotation / of Q, against the minimiser's
  t, X, T largest |difference| of an entry of c_translation / position / T, relative to the largest |entry| of the minimiser's
          (X without the points of a single observation: their depth is not determined by the problem; KKT covers them)
  kkt     largest |entry| of the Gauss-Newton step computed in numpy AT the returned state, relative to the largest |position|
  dcost, dradius  (default options) largest relative difference, over the iterations, of the trace's cost / trust_region_radius
          from the restatement's trace

BARS.  bar = 16 x the worst value the numpy restatement reaches against the same 50-digit fixtures, per metric and regime, floor 2,
as tests/test_pnp.py has it; REF below is that measurement, and test_restatement_holds_its_record re-measures it.  The regimes are
those of the generator's list: f2 (F = 2, P = 6), f3 (F = 3, P = 8, l = 0 and 1), f11_full (F = 11, P = 60, full tracks: plain,
wide, exact, the far start), f11_rag (ragged, l = 0, 4, 9) and f11_big (P = 65 and 257).
Near the minimiser the ratio rho is rounding noise: which steps a double-precision run still accepts differs from run to run, and the
state it ends in is only as close to the minimiser as sqrt(eps x cost / curvature) — that is what REF's R .. kkt record, and why (b)
holds the final state and never the termination type.  (On f11_full the restatement happens to accept one more step, whose cost
change is 2 units in the last place of the cost, and ends 35 x closer than the device, which sees a cost change of exactly 0 there and
converges: the same policy on the same numbers up to rounding; the regime's worst is another of its cases.)
For dcost / dradius there is no 50-digit trace; the restatement's own error is measured as the spread between its trace on the stored
fixture and its traces on four other listings of the same problem (the points reversed, and in three shuffled orders: the same
mathematics, other rounding), and the device is held to bar + that spread = 17 x it (floor 2 + the spread).  The trace test runs on
every case but the one with exact bearings (the issue keeps that one for the evaluation).  The generator's seeds are chosen so that
each of them keeps clear of the loop's thresholds by a factor 2: every relative_decrease, the |cost_change| / cost of every valid step
(accepted or rejected) and of the step that ends the run, which the trace does not hold.

worst restatement / bar / worst device (MI355X), per regime
  regime    cost0                         gmax0                         R                             t                             X
  f2        1.5/24/0.72                   5.1/81.6/5.1                  4.5e+06/7.2e+07/1e+06         0/2/0                         1.2e+07/1.92e+08/2.7e+06
  f3        2/32/1.9                      3.9/62.4/4.8                  6.2e+05/9.92e+06/6.2e+05      6e+05/9.6e+06/6e+05           1.9e+06/3.04e+07/1.8e+06
  f11_full  1.5/24/1.5                    0.52/8.32/1                   1.2e+05/1.92e+06/4.7e+05      2.6e+05/4.16e+06/8.8e+05      2e+05/3.2e+06/2.6e+06
  f11_rag   1.5/24/1.4                    2.3/36.8/1.5                  2.5e+07/4e+08/3.9e+06         2e+08/3.2e+09/1.9e+07         4.1e+08/6.56e+09/3.8e+07
  f11_big   0.62/9.92/0                   1.3/20.8/2.5                  1.4e+06/2.24e+07/1.2e+06      3.6e+06/5.76e+07/3.5e+06      7e+07/1.12e+09/7e+07
  regime    RQ                            T                             kkt                           dcost                         dradius
  f2        4.5e+06/7.2e+07/1e+06         4.5e+06/7.2e+07/1e+06         1.4e+07/2.24e+08/3.2e+06      6.5e+03/1.04e+05/7.9e+02      0/2/0
  f3        6.2e+05/9.92e+06/6.2e+05      6.3e+05/1.01e+07/6.2e+05      2.3e+06/3.68e+07/2.3e+06      3.9e+02/6.24e+03/3.6e+02      0/2/0
  f11_full  1.2e+05/1.92e+06/4.7e+05      2.6e+05/4.16e+06/8.9e+05      1.9e+05/3.04e+06/2.6e+06      1.4e+03/2.24e+04/1.4e+03      0/2/0
  f11_rag   2.5e+07/4e+08/3.9e+06         2e+08/3.2e+09/1.9e+07         6.4e+08/1.02e+10/5.4e+07      1.8e+04/2.88e+05/4e+03        5.3e+06/8.48e+07/2.7e+06
  f11_big   1.4e+06/2.24e+07/1.2e+06      3.5e+06/5.6e+07/3.5e+06       7.1e+07/1.14e+09/7e+07        2.9e+02/4.64e+03/2.6e+02      0/2/0
"""
import ctypes as C
import os

import numpy as np
import pytest

import sfm_ba_ref as sr
from golden import gen_sfm_ba_hp as gen

EPS = 2.0 ** -52
FACTOR, FLOOR = 16.0, 2.0
A_METRICS, B_METRICS, D_METRICS = ("cost0", "gmax0"), ("R", "t", "X", "RQ", "T", "kkt"), ("dcost", "dradius")
CASES = ("f2_p6", "f3_p8_l0", "f3_p8_l1", "f11_full", "f11_full_wide", "f11_full_exact", "f11_full_reject", "f11_rag_l0", "f11_rag_l4", "f11_rag_l9",
         "f11_rag_p65", "f11_rag_p257")
B_CASES = tuple(c for c in CASES if c != "f11_full_exact")  # exact bearings: evaluation only
D_CASES = B_CASES  # the trace test: every case with noisy bearings; the seeds are chosen so that their margins hold (test_fixture_conditions)
FORCE = gen.FORCE

REGIME = {"f2_p6": "f2", "f3_p8_l0": "f3", "f3_p8_l1": "f3", "f11_full": "f11_full", "f11_full_wide": "f11_full", "f11_full_exact": "f11_full",
          "f11_full_reject": "f11_full", "f11_rag_l0": "f11_rag", "f11_rag_l4": "f11_rag", "f11_rag_l9": "f11_rag", "f11_rag_p65": "f11_big", "f11_rag_p257": "f11_big"}
REGIMES = ("f2", "f3", "f11_full", "f11_rag", "f11_big")

# worst value of the numpy restatement against the 50-digit fixtures, per regime (rounded up to two digits)
REF = {
    "f2": dict(cost0=1.5, gmax0=5.1, R=4.5e+06, t=0, X=1.2e+07, RQ=4.5e+06, T=4.5e+06, kkt=1.4e+07, dcost=6.5e+03, dradius=0),
    "f3": dict(cost0=2, gmax0=3.9, R=6.2e+05, t=6e+05, X=1.9e+06, RQ=6.2e+05, T=6.3e+05, kkt=2.3e+06, dcost=3.9e+02, dradius=0),
    "f11_full": dict(cost0=1.5, gmax0=0.52, R=1.2e+05, t=2.6e+05, X=2e+05, RQ=1.2e+05, T=2.6e+05, kkt=1.9e+05, dcost=1.4e+03, dradius=0),
    "f11_rag": dict(cost0=1.5, gmax0=2.3, R=2.5e+07, t=2e+08, X=4.1e+08, RQ=2.5e+07, T=2e+08, kkt=6.4e+08, dcost=1.8e+04, dradius=5.3e+06),
    "f11_big": dict(cost0=0.62, gmax0=1.3, R=1.4e+06, t=3.6e+06, X=7e+07, RQ=1.4e+06, T=3.5e+06, kkt=7.1e+07, dcost=2.9e+02, dradius=0),
}


def bar(case, metric):
    return max(FACTOR * REF[REGIME[case]][metric], FLOOR)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "sfm_ba_hp.npz"))
    fx = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["names"]}
    for f in fx.values():
        f["pb"] = sr.problem(int(f["F"]), int(f["l"]), f["off"], f["frame"], f["bearing"])
    return fx


def restatement(f, **opt):
    return sr.solve(f["pb"], f["q0"], f["t0"], f["X0"], **opt)


def device(eng):
    return lambda f, **opt: eng.sfm_ba(int(f["l"]), f["off"], f["frame"], f["bearing"], f["q0"], f["t0"], f["X0"], **opt)


def rot(q):
    return sr.rotation(np.asarray(q, np.float64), sr.F64)


def metrics_a(got, f):
    return dict(cost0=abs(got["initial_cost"] - float(f["cost0"])) / (EPS * float(f["cost0"])),
                gmax0=abs(got["trace"][0]["gradient_max_norm"] - float(f["gmax0"])) / (EPS * float(f["gmax0"])))


def kkt(got, f):
    with np.errstate(all="ignore"):
        dc, dp = sr.gauss_newton_step(f["pb"], got["c_rotation"], got["c_translation"], got["position"], sr.F64, f["active_c"], f["single"])
    return float(max(np.abs(dc).max(), np.abs(dp).max()) / (EPS * np.abs(f["X_min"]).max()))


def metrics_b(got, f):
    keep = ~f["single"]
    rel = lambda a, b: float(np.abs(np.asarray(a) - b).max() / (EPS * np.abs(b).max()))
    return dict(R=float(np.abs(rot(got["c_rotation"]) - f["R_min"]).max() / EPS), t=rel(got["c_translation"], f["t_min"]),
                X=rel(got["position"][keep], f["X_min"][keep]), RQ=float(np.abs(rot(got["Q"]) - f["RQ_min"]).max() / EPS), T=rel(got["T"], f["T_min"]),
                kkt=kkt(got, f))


def trace_spread(a, b):
    """Largest relative difference of cost and trust_region_radius over two traces of equal length, in eps."""
    assert len(a) == len(b)
    return dict(dcost=max(abs(x["cost"] - y["cost"]) / (EPS * y["cost"]) for x, y in zip(a, b)),
                dradius=max(abs(x["trust_region_radius"] - y["trust_region_radius"]) / (EPS * y["trust_region_radius"]) for x, y in zip(a, b)))


def listings(f):
    """Five orders of the points of one problem: as stored, reversed, and three shuffles.  The same mathematics, other rounding."""
    P = len(f["off"]) - 1
    return [np.arange(P), np.arange(P)[::-1]] + [np.random.default_rng(s).permutation(P) for s in (1, 2, 3)]


def relisted(f, perm):
    """The case with its points listed in the order perm (the fixture's per-point records follow)."""
    off = f["off"]
    order = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm])
    o2 = np.concatenate([[0], np.cumsum(np.diff(off)[perm])]).astype(np.int32)
    g = dict(f)
    g.update(off=o2, frame=f["frame"][order], bearing=f["bearing"][order], X0=f["X0"][perm], X_min=f["X_min"][perm], single=f["single"][perm])
    g["pb"] = sr.problem(int(f["F"]), int(f["l"]), o2, g["frame"], g["bearing"])
    return g


def check(m, case, tag):
    bad = [f"{tag} {case} {k}: {v:.3g} > bar {bar(case, k):.3g}" for k, v in m.items() if not v <= bar(case, k)]
    assert not bad, "\n".join(bad)


def show(tag, case, m):
    print(f"  {tag} {case:16s} " + " ".join(f"{k} {v:9.3g}" for k, v in m.items()))


def worst(ms):
    return {k: max(m[k] for m in ms) for k in ms[0]}


def measure_restatement(fx):
    """Per regime, the worst over its cases of: the evaluation and the forced-convergence result on the stored fixture; the spread of the
    default-option trace between the stored listing and four other listings of the same problem."""
    out = {}
    for case in CASES:
        f = fx[case]
        m = metrics_a(restatement(f, max_num_iterations=0), f)
        if case in B_CASES:
            m.update(metrics_b(restatement(f, **FORCE), f))
        if case in D_CASES:
            ref = restatement(f)["trace"]
            m.update(worst([trace_spread(restatement(relisted(f, p))["trace"], ref) for p in listings(f)[1:]]))
        r = out.setdefault(REGIME[case], {})
        for k, v in m.items():
            r[k] = max(r.get(k, 0.0), v)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_conditions(fixtures):
    """CPU: the file holds the regimes it is meant to, the tangent Jacobian at the minimiser has a condition number <= 1e6 (over what the
    problem determines), and the restatement's default-option trace of every case of the trace test keeps clear of the two thresholds:
    every relative_decrease outside [0.5e-3, 2e-3], every accepted |cost_change| / cost outside [0.5e-6, 2e-6]."""
    assert set(fixtures) == set(CASES)
    shape = lambda c: (int(fixtures[c]["F"]), len(fixtures[c]["off"]) - 1, int(fixtures[c]["l"]))
    assert shape("f2_p6") == (2, 6, 0) and shape("f3_p8_l0") == (3, 8, 0) and shape("f3_p8_l1") == (3, 8, 1)
    assert [shape(c)[2] for c in ("f11_rag_l0", "f11_rag_l4", "f11_rag_l9")] == [0, 4, 9]
    assert shape("f11_rag_p65")[:2] == (11, 65) and shape("f11_rag_p257")[:2] == (11, 257)
    assert all(np.all(np.diff(fixtures[c]["off"]) == 11) for c in CASES if c.startswith("f11_full"))
    assert not np.any(fixtures["f11_rag_l4"]["frame"] == 7) and np.diff(fixtures["f11_rag_l0"]["off"])[0] == 1
    z = fixtures["f11_full_wide"]["bearing"][:, 2]
    assert np.any(z < -0.1) and np.any(z > 0.1)
    assert np.abs(np.linalg.norm(fixtures["f11_rag_l9"]["bearing"], axis=1) - 1).max() > 1e-3
    assert float(fixtures["f11_full_exact"]["cost_min"]) < 1e-28  # (the bearings are rounded to double: M eps^2)
    for case in B_CASES:
        f = fixtures[case]
        got = restatement(f, **FORCE)
        cond = gen.condition(f["pb"], f, got["c_rotation"], got["c_translation"], got["position"])
        print(f"  {case:16s} cond {cond:.3g} (generator: {float(f['cond']):.3g})")
        assert cond <= gen.COND_CAP and float(f["cond"]) <= gen.COND_CAP, case
    for case in D_CASES:
        assert gen.margins(restatement(fixtures[case])) == (True, True), case
        assert int(fixtures[case]["rho_margin_ok"]) == 1 and int(fixtures[case]["dcost_margin_ok"]) == 1


def test_restatement_holds_its_record(fixtures):
    """CPU: the numpy restatement against the 50-digit fixtures is what REF says (REF is rounded up to two digits), on every metric."""
    got = measure_restatement(fixtures)
    for r in REGIMES:
        print(f'    "{r}": dict(' + ", ".join(f"{k}={v:.2g}" for k, v in got[r].items()) + "),")
    for r in REGIMES:
        assert set(got[r]) == set(REF[r]), r
        for k, v in got[r].items():
            assert v <= REF[r][k] * (1 + 1e-9), (r, k, v, REF[r][k])
            assert v >= 0.5 * REF[r][k] or REF[r][k] <= 1.0, f"REF[{r}][{k}] = {REF[r][k]} is stale: measured {v}"


def test_restatement_evaluation_against_the_fixtures(fixtures):
    """CPU: gradient and reduced camera system of the restatement at the start against the 50-digit ones.  Every entry is a sum of at
    most M products of rounded factors: held to 8 M eps x the largest entry of the quantity."""
    for case in CASES:
        f = fixtures[case]
        pb = f["pb"]
        ev = sr.evaluate(pb, f["q0"], f["t0"], f["X0"])
        gc, gp = sr.gradient(pb, ev)
        sc, sp = sr.jacobi_scale(pb, ev)
        sch = sr.schur(pb, sr.blocks(pb, ev, sc, sp), sr.INITIAL_RADIUS)
        tol = 8 * pb["M"] * EPS
        for name, a, b in (("gc", gc, f["gc0"]), ("gp", gp, f["gp0"]), ("S", sch["S"], f["S0"]), ("rhs", sch["rhs"], f["rhs0"])):
            assert np.abs(a - b).max() <= tol * np.abs(b).max(), (case, name, np.abs(a - b).max() / np.abs(b).max())


def test_analytic_jacobian_against_a_50_digit_derivative(fixtures):
    """CPU: N (-2 [R X]x), N, N R against a central difference of the literal residual in 50 digits (the generator's own check, on one case)."""
    f = fixtures["f3_p8_l1"]
    assert gen.check_jacobian(f["pb"], f) < 1e-30


def test_fixtures_are_the_generators(fixtures):
    """CPU: the inputs of one case re-made by the generator, bit for bit, and its 50-digit evaluation."""
    f = fixtures["f2_p6"]
    sc = gen.make_scene(**gen.CASES["f2_p6"])
    for k in ("off", "frame", "bearing", "q0", "t0", "X0"):
        assert np.array_equal(sc[k], f[k]), k
    ev = sr.evaluate(f["pb"], f["q0"], f["t0"], f["X0"], sr.HP)
    assert float(ev["cost"]) == float(f["cost0"])


def test_scipy_moves_nothing(fixtures):
    """CPU: scipy's least_squares on the tangent parametrisation (delta -> r(x [+] delta)), started at the restatement's forced-
    convergence result, moves no metric by more than the bar of (b)."""
    from scipy.optimize import least_squares

    for case in ("f2_p6", "f3_p8_l1", "f11_full"):
        f = fixtures[case]
        pb = f["pb"]
        got = restatement(f, **FORCE)
        q, t, X = got["c_rotation"], got["c_translation"], got["position"]
        fr, k6 = np.nonzero(pb["col"] >= 0)

        def moved(x):
            dc = np.zeros((pb["F"], 6))
            dc[fr, k6] = x[:pb["n"]]
            return sr.plus(q, t, X, dc, x[pb["n"]:].reshape(-1, 3))

        fun = lambda x: sr.evaluate(pb, *moved(x), jac=False)["r"].reshape(-1)
        jac = lambda x: sr.dense_jacobian(pb, sr.evaluate(pb, *moved(x)))  # (the tangent Jacobian at x [+] delta: exact at delta = 0)
        res = least_squares(fun, np.zeros(pb["n"] + 3 * pb["P"]), jac=jac, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15)
        q2, t2, X2 = moved(res.x)
        m = dict(R=float(np.abs(rot(q2) - rot(q)).max() / EPS), t=float(np.abs(t2 - t).max() / (EPS * np.abs(t).max())), X=float(np.abs(X2 - X).max() / (EPS * np.abs(X).max())))
        show("scipy", case, m)
        check(m, case, "scipy")


def failure_case(fixtures):
    """A start that no step can leave: point 0 lies 1e-158 from the centre of frame l (whose blocks are constant), the squared norm of
    its Jacobian columns overflows, its Jacobi scale is 0 and its block 0 x inf.  The cost is finite (every residual is at most 2)."""
    f = dict(fixtures["f3_p8_l0"])
    f["t0"], f["X0"] = f["t0"].copy(), f["X0"].copy()
    f["t0"][0] = 0.0
    f["X0"][0] = (1e-158, 0.0, 0.0)
    return f


def test_restatement_fails_on_the_failure_case(fixtures):
    """CPU: five invalid steps in a row end the restatement with FAILURE and the start as the state."""
    f = failure_case(fixtures)
    got = restatement(f)
    assert got["termination"] == sr.FAILURE and got["num_iterations"] == 5 and np.array_equal(got["position"], f["X0"])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_a_evaluation(eng, fixtures):
    """(a): with max_num_iterations = 0, initial_cost and iteration 0's gradient_max_norm against the 50-digit values; the state comes back
    bit for bit."""
    for case in CASES:
        f = fixtures[case]
        got = device(eng)(f, max_num_iterations=0)
        assert got["num_iterations"] == 1 and got["termination"] == sr.NO_CONVERGENCE and got["final_cost"] == got["initial_cost"], case
        assert np.array_equal(got["c_rotation"], f["q0"]) and np.array_equal(got["c_translation"], f["t0"]) and np.array_equal(got["position"], f["X0"]), case
        m = metrics_a(got, f)
        show("device (a)", case, m)
        check(m, case, "(a)")


@pytest.mark.gpu
@pytest.mark.parametrize("case", B_CASES)
def test_b_minimiser_and_c_kkt(eng, fixtures, case):
    """(b) and (c): with the three tolerances forced far below their defaults, the final state, Q and T against the 50-digit minimiser, and
    the Gauss-Newton step computed on the CPU at the returned state.  f11_full_reject starts 12 degrees / 0.2 / 30 % away.  The constant
    blocks, and the blocks of a frame with no observation, come back bit for bit."""
    f = fixtures[case]
    got = device(eng)(f, **FORCE)
    m = metrics_b(got, f)
    show("device (b, c)", case, m)
    check(m, case, "(b, c)")
    l, F = int(f["l"]), int(f["F"])
    assert np.array_equal(got["c_rotation"][l], f["q0"][l]) and np.array_equal(got["c_translation"][[l, F - 1]], f["t0"][[l, F - 1]])
    for fr in np.nonzero(~f["active_c"][:, 0])[0]:
        assert np.array_equal(got["c_rotation"][fr], f["q0"][fr]) and np.array_equal(got["c_translation"][fr], f["t0"][fr])
    assert got["accepted"] == int(got["termination"] == sr.CONVERGENCE or got["final_cost"] < 5e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", D_CASES)
def test_d_default_options_against_the_restatement(eng, fixtures, case):
    """(d): against the RESTATEMENT of the loop policy (parity with Ceres itself is not pinned): the same number of
    iterations, the same accepted and rejected steps, termination and `accepted`; cost and radius per iteration within bar + the
    restatement's own spread."""
    f = fixtures[case]
    got, ref = device(eng)(f), restatement(f)
    for k in ("num_iterations", "termination", "accepted", "num_successful_steps", "num_unsuccessful_steps"):
        assert got[k] == ref[k], (case, k, got[k], ref[k])
    assert [it["step_is_successful"] for it in got["trace"]] == [it["step_is_successful"] for it in ref["trace"]]
    assert [it["step_is_valid"] for it in got["trace"]] == [it["step_is_valid"] for it in ref["trace"]]
    m = trace_spread(got["trace"], ref["trace"])
    show("device (d)", case, m)
    own = REF[REGIME[case]]
    bad = [f"{case} {k}: {v:.3g} > {bar(case, k) + own[k]:.3g}" for k, v in m.items() if not v <= bar(case, k) + own[k]]
    assert not bad, "\n".join(bad)


def same_bits(a, b):
    keys = ("c_rotation", "c_translation", "position", "Q", "T")
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["trace"] == b["trace"] and all(a[k] == b[k] for k in ("termination", "num_iterations", "final_cost", "accepted"))


@pytest.mark.gpu
def test_a_repeated_call_returns_the_same_bits(eng, fixtures):
    for case in ("f2_p6", "f11_rag_l4", "f11_rag_p257"):
        f = fixtures[case]
        a, b = device(eng)(f), device(eng)(f)
        assert a["num_iterations"] > 1 and same_bits(a, b), case


@pytest.mark.gpu
def test_drop_in_identity(eng, fixtures):
    """Q and T are initial_sfm.cpp:295-309 applied on the CPU to the returned c_rotation, c_translation, to 2 eps (T: x the largest |t|)."""
    for case in ("f3_p8_l1", "f11_rag_l9"):
        f = fixtures[case]
        got = device(eng)(f)
        Q, T = sr.drop_in(got["c_rotation"], got["c_translation"])
        assert np.abs(got["Q"] - Q).max() <= 2 * EPS and np.abs(got["T"] - T).max() <= 2 * EPS * np.abs(got["c_translation"]).max(), case


def filled():
    from lfvio import abi

    out = abi.SfmBaOutC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return out


@pytest.mark.gpu
def test_five_invalid_steps_end_in_failure(eng, fixtures):
    """Zero bearings do NOT make a start fail (the gradient is zero up to rounding and the first tiny step converges); a point 1e-158
    from a camera centre does: every step is non-finite, five in a row return LFVIO_FAILURE with the start as the state."""
    f = failure_case(fixtures)
    got = device(eng)(f)
    assert got["termination"] == sr.FAILURE and got["num_iterations"] == 5 and got["accepted"] == 0
    assert [it["step_is_valid"] for it in got["trace"]] == [0] * 5
    assert np.array_equal(got["position"], f["X0"]) and np.array_equal(got["c_rotation"], f["q0"]) and np.array_equal(got["c_translation"], f["t0"])


@pytest.mark.gpu
def test_errors_leave_the_outputs_alone(eng, fixtures):
    """Every LFVIO_ERR_ARG case and the non-finite initial cost."""
    from lfvio import abi

    f = fixtures["f3_p8_l0"]
    l, off, frm, us, q, t, X = int(f["l"]), f["off"], f["frame"], f["bearing"], f["q0"], f["t0"], f["X0"]
    big = 4097
    twice = frm.copy()
    twice[1] = twice[0]
    bad_off = off.copy()
    bad_off[2] = bad_off[1]
    cases = {
        "F = 1": (0, [0, 1], [0], us[:1], q[:1], t[:1], X[:1], {}),
        "F = 12": (0, off, frm, us, np.tile(q, (4, 1)), np.tile(t, (4, 1)), X, {}),
        "l = -1": (-1, off, frm, us, q, t, X, {}),
        "l = F - 1": (2, off, frm, us, q, t, X, {}),
        "P = 4097": (l, np.arange(big + 1), np.zeros(big, np.int32), np.tile(us[:1], (big, 1)), q, t, np.tile(X[:1], (big, 1)), {}),
        "offset[0] != 0": (l, off + 1, frm, np.concatenate([us[:1], us]), q, t, X, {}),
        "a point with no observation": (l, bad_off, frm, us, q, t, X, {}),
        "a point with F + 1": (l, [0, 4], [0, 1, 2, 1], us[:4], q, t, X[:1], {}),
        "frame = F": (l, off, np.where(np.arange(len(frm)) == 5, 3, frm), us, q, t, X, {}),
        "frame = -1": (l, off, np.where(np.arange(len(frm)) == 5, -1, frm), us, q, t, X, {}),
        "a frame twice": (l, off, twice, us, q, t, X, {}),
        "64 iterations": (l, off, frm, us, q, t, X, dict(max_num_iterations=64)),
    }
    nan_X = X.copy()
    nan_X[3, 1] = np.nan
    cases_nonfinite = {"NaN position": (l, off, frm, us, q, t, nan_X, {})}
    for want, group in ((-1, cases), (-3, cases_nonfinite)):
        for tag, (l_, o_, f_, u_, q_, t_, X_, opt) in group.items():
            out = filled()
            before = bytes(out)
            got = eng.sfm_ba(l_, o_, f_, u_, q_, t_, X_, out=out, check=False, **opt)
            assert got["rc"] == want and bytes(out) == before, tag
            same = lambda a, b: np.array_equal(np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1), equal_nan=True)
            assert same(got["c_rotation"], q_) and same(got["c_translation"], t_) and same(got["position"], X_), tag
    out = filled()
    before = bytes(out)
    bin_ = abi.SfmBaInC()
    bin_.num_frames, bin_.ref_frame, bin_.num_points, bin_.max_num_iterations = 3, 0, 8, -1
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    qc, tc, Xc = q.copy(), t.copy(), X.copy()
    assert eng.lib.lfvio_sfm_ba(eng.ctx, C.byref(bin_), dp(qc), dp(tc), dp(Xc), C.byref(out)) == -1  # null arrays
    assert eng.lib.lfvio_sfm_ba(eng.ctx, None, dp(qc), dp(tc), dp(Xc), C.byref(out)) == -1
    ip = C.POINTER(C.c_int)
    o32, f32 = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(frm, np.int32)
    bin_.obs_offset, bin_.obs_frame, bin_.obs_bearing = o32.ctypes.data_as(ip), f32.ctypes.data_as(ip), dp(us)
    assert eng.lib.lfvio_sfm_ba(eng.ctx, C.byref(bin_), None, dp(tc), dp(Xc), C.byref(out)) == -1
    assert eng.lib.lfvio_sfm_ba(eng.ctx, C.byref(bin_), dp(qc), dp(tc), dp(Xc), None) == -1
    assert bytes(out) == before and np.array_equal(qc, q) and np.array_equal(tc, t) and np.array_equal(Xc, X)
    assert device(eng)(f)["rc"] == 0  # the context is still good
