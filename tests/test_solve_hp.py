"""The dense solve of one trust-region pass (k_solve_dense, csrc/kernels_solve.h) and the Schur phase of the landmark sweep against
a 50-digit reference (tests/solve_hp.py).

Every other test sees the solve through the end of a call (states 1e-6, costs 1e-7) or against a second device path that shares the
same Cholesky (test_linw.py, 1e-6).  Here one pass is run (lfvio_debug_pass_io) and what the solve WROTE is held to a 50-digit
statement of Ceres' formulas evaluated on what the solve READ: the backward and forward error of the Gauss-Newton step, scale /
diagonal_ / gradient_ entry by entry, alpha and the quadratic forms of the dogleg model, the Schur sums entry by entry, and the exact
properties.  For the assembling form (a resident batch behind k_linw) H_pp is put together by solve_hp.assemble_hp from the three
sources the kernel scatters.

Bars: 16 x the worst of three double-precision comparators (LAPACK, a textbook Cholesky in numpy loops, the oracle's schur_solve) on the
same cases, measured and asserted in the CPU tests below (solve_hp.COMPARATOR_WORST); nothing is taken from the device.
A bar belongs to a metric and a case class (group, mu) — see GROUP below; the metrics in units of eps that involve neither y nor the
conditioning are pooled over all classes (solve_hp.POOLED).  Measured, worst of the class, comparators / bar / device (MI355X, both
routes: k_lin + k_sum -> k_solve_dense<false> and the resident batch k_linw -> k_solve_dense<true>):

  class            eta (eps)        fwd (eps kappa)       Q_GN (eps kappa)          Q_NN (eps kappa)          Q_GN_SQ (eps kappa)
  regular 1e-8     0.62/9.9/0.49    0.91/14.6/0.85        2.1e-8/3.3e-7/6.1e-9      4.6e-8/7.4e-7/1.4e-8      0.20/3.2/0.082
  regular 1e-5     0.48/7.7/0.64    0.93/14.9/0.98        1.0e-5/1.6e-4/7.7e-6      2.0e-5/3.3e-4/1.5e-5      1.7e-3/0.028/3.1e-3
  regular 1e-2     0.66/10.5/0.44   1.29/20.6/0.84        0.015/0.25/0.0034         0.029/0.47/0.0062         0.15/2.4/0.13
  regular 0.5      0.65/10.3/0.54   2.54/40.6/1.71        0.61/9.8/0.37             0.80/12.8/0.32            1.13/18.1/0.94
  weak 1e-8        0.30/4.8/0.23    3.1e-3/0.050/1.9e-3   9.0e-4/0.014/5.6e-4       1.6e-3/0.026/9.3e-4       2.3e-3/0.037/1.9e-3
  prior 1e-8       0.21/3.4/0.20    0.30/4.7/0.22         0.050/0.80/0.13           0.073/1.17/0.18           0.077/1.2/0.19
  prior 1e-5       0.31/5.0/0.23    0.40/6.5/0.33         8.3e-3/0.13/8.5e-3        3.4e-3/0.054/2.8e-3       0.19/3.1/0.046
  prior 1e-2       0.59/9.4/0.32    1.72/27.5/0.71        0.14/2.3/0.035            0.38/6.1/0.032            2.9/46.7/1.15
  prior 0.5        0.28/4.5/0.20    0.78/12.5/0.77        0.82/13.1/0.13            0.77/12.3/1.18            0.88/14.0/0.46
  (alpha, Q_gN, Q_GRAD_GN: the device between 0.2 x and 6 x the comparators in every class, bars at 16 x; the lines the tests print)

  pooled, in eps   scale 1.66/26.6/1.87   diagonal_ 2.11/33.8/2.03   gradient_ 2.45/39.2/2.68   uc_grad 3.71/59.4/4.10
                   Q_GG 4.32/69.1/2.88    Q_gG 1.93/30.9/2.11        Q_GRAD_SQ 1.68/26.9/3.63
  Schur sums, eps of the sum of the absolute terms:   C 9.8/157/10.6   z1 3.5/55/3.2   z2 4.3/68/3.8   ls1 7.6/122/1.7   ls2 7.6/122/2.1

The device is as close to the truth as LAPACK on the rounded system: its backward error is 0.2 - 0.6 eps everywhere, and the forms it
derives from identities (N^T H N = |z|^2 - mu |gn|^2 + N_c^T C N_c, ...) are as good as x^T H x over the whole matrix in double.

Cases replaced after the CPU preconditions (kappa eps < 1e-3), none left out: the IMU-only window, the static window and the window
without its first IMU factor each had a column that nothing but mu D^2 = 1e-14 holds (ex / td without a landmark, td at rest, speed /
bias 0 without its factor and without a prior: kappa eps = 0.04); they run with ex and td constant, with td constant, and with a prior.
What the checks cannot see, shown on the CPU: one Newton step on a reciprocal estimate good to 2^-26 (2 eps per reciprocal: eta 0.17,
the comparators' own), and the mu terms of Q_NN / Q_GN in the weak class at mu = 1e-8, where the terms are 1e-3 .. 1e-2 of eps kappa.
"""
import numpy as np
import pytest

from lfvio import abi

import solve_hp as sh
from solve_cases import CASES, GROUP, case_class, window  # noqa: F401  (shared with tests/test_step_hp.py)

MU0 = 1e-8
MUS_MORE = (1e-5, 1e-2, 0.5)


BENCH = "bench"
NAMES = list(CASES)
RUNS = [(n, mu) for n in NAMES for mu in ((MU0,) + MUS_MORE if CASES[n][1] else (MU0,))]
ROLES, LINW = 0, 2  # lfvio_debug_configure "linw": k_lin + k_sum -> k_solve_dense<false> | k_linw -> k_solve_dense<true>
DEVICE_NAMES = {ROLES: [n for n in NAMES if n != BENCH], LINW: NAMES}
DEVICE_RUNS = [(r, n, mu) for r in (ROLES, LINW) for n, mu in RUNS if n in DEVICE_NAMES[r]]
DEVICE_CASES = [(r, n) for r in (ROLES, LINW) for n in DEVICE_NAMES[r]]


def _rid(v):
    return "-".join(("roles" if x == ROLES else "linw") if isinstance(x, int) else f"{x:g}" if isinstance(x, float) else x for x in v)


def _line(tag, ref, rep, cls):
    worst = max(sh.Q_NAMES + ("alpha",), key=lambda k: rep[k] / max(sh.bar(k, cls), 1e-300))  # (the one closest to its bar)
    return (f"{tag}: kappa={ref.kappa:.2e} cert={ref.cert:.0e}/{ref.steps} eta={rep['eta']:.3g} fwd={rep['fwd']:.3g} scale={rep['scale']:.2f} "
            f"diag={rep['diag']:.2f} grad={rep['grad']:.2f} uc_grad={rep['uc_grad']:.2f} worst scalar {worst}={rep[worst]:.3g}  all: "
            + " ".join(f"{k}={rep[k]:.3g}" for k in ("alpha",) + sh.Q_NAMES))


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the oracle's blocks as inputs
# ------------------------------------------------------------------------------------------------------------------------
_cpu = {}


def cpu_reference(oracle, name, mu):
    """The 50-digit reference on the oracle's linearization of the case, and the three comparators' reports: computed once."""
    key = (name, mu)
    if key not in _cpu:
        w = window(oracle, name)
        lin = oracle.linearize(w)
        sch = sh.schur_hp(lin["a"], lin["b"], lin["W"], mu)
        ref = sh.Reference(lin["H"], lin["g"], sch["C"], sch["z1"], mu, sh.active_columns(w.estimate_extrinsic, w.estimate_td), sch)
        ys = dict(lapack=sh.lapack_solve(ref.Sd, ref.rhs_d), textbook=sh.textbook_solve(ref.Sd, ref.rhs_d), oracle=oracle.schur_step(w, mu)[:sh.KP])
        _cpu[key] = dict(w=w, lin=lin, sch=sch, ref=ref, ys=ys, reps={k: ref.report(sh.comparator_outputs(ref, y)) for k, y in ys.items()})
    return _cpu[key]


@pytest.mark.parametrize("name,mu", RUNS, ids=[_rid(v) for v in RUNS])
def test_preconditions_and_comparators_inside_every_bar(oracle, name, mu):
    """solve_hp certifies, LAPACK factors, kappa eps < 1e-3; the three comparators through every metric of the step (this is where
    the bars come from: the printed figures are what solve_hp.COMPARATOR_WORST holds)."""
    R = cpu_reference(oracle, name, mu)
    ref = R["ref"]
    assert ref.cert < sh.CERTIFICATE and ref.kappa * sh.EPS < 1e-3, (ref.cert, ref.kappa)
    for k, rep in R["reps"].items():
        print(_line(f"{name} mu={mu:g} {k}", ref, rep, case_class(name, mu)))
    for k, rep in R["reps"].items():
        assert sh.failed_checks(rep, sh.STEP_METRICS, case_class(name, mu)) == [], k


@pytest.mark.parametrize("name,mu", RUNS, ids=[_rid(v) for v in RUNS])
def test_schur_sums_in_double_are_inside_the_bars(oracle, name, mu):
    """numpy in double, in landmark order and reversed, against schur_hp: entry by entry over the sum of the absolute terms."""
    R = cpu_reference(oracle, name, mu)
    lin, N = R["lin"], R["w"].N
    for tag, order in (("forward", None), ("reversed", range(N - 1, -1, -1))):
        rep = sh.schur_report(sh.schur_double(lin["a"], lin["b"], lin["W"], mu, order), R["sch"])
        print(f"{name} mu={mu:g} schur {tag}: " + " ".join(f"{k}={rep[k]:.2f}" for k in sh.SCHUR_METRICS))
        assert sh.failed_checks(rep, sh.SCHUR_METRICS, case_class(name, mu)) == []


def oracle_sources(oracle, w):
    """The three sources of the assembling solve from the oracle's own factor blocks: the visual terms of the camera part (the
    linearization of the window without its IMU factors and prior), the 30 x 30 blocks J^T J of the IMU factors, the prior's J0^T J0."""
    off = []
    for p in w.imu:
        q = abi.preint_from_array(abi.preint_to_array(p))
        q.sum_dt = 1e9
        off.append(q)
    vis = oracle.linearize(w.copy(imu=off, prior=None))["H"]
    assert np.abs(vis[sh.KC:]).max() == 0.0
    blocks = np.zeros((10, 30, 30))
    for f in range(10):
        if w.imu[f].sum_dt > 10.0:
            continue
        _, Jpi, Jsi, Jpj, Jsj, _ = oracle.imu_evaluate(w.imu[f], w.g, w.pose[f], w.speed_bias[f], w.pose[f + 1], w.speed_bias[f + 1])
        J = np.hstack([Jpi[:, :6], Jsi, Jpj[:, :6], Jsj])
        blocks[f] = J.T @ J
    if w.prior is not None and w.prior.valid:
        J0 = w.prior.J()
        return vis[:sh.KC, :sh.KC], blocks, J0.T @ J0, sh.prior_column_map(w.prior)
    return vis[:sh.KC, :sh.KC], blocks, np.zeros((0, 0)), np.zeros(0, np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_assemble_hp_is_the_oracles_matrix(oracle, name):
    """assemble_hp fed the oracle's own factor blocks equals oracle.linearize's H at 1e-13 (of the largest entry of the row and the
    column): the index maps are pinned independently of the device."""
    w = window(oracle, name)
    H = sh.to_f(sh.assemble_hp(*oracle_sources(oracle, w), w.estimate_extrinsic, w.estimate_td))
    Ho = oracle.linearize(w)["H"]
    d = np.sqrt(np.maximum(np.abs(np.diag(Ho)), 1e-300))
    assert (np.abs(H - Ho) / (d[:, None] * d[None, :])).max() < 1e-13
    assert np.array_equal(H != 0, Ho != 0)


@pytest.mark.parametrize("name", NAMES)
def test_schur_hp_and_reduced_hp_agree_with_the_oracles_schur_step(oracle, name):
    """The 50-digit y of schur_hp + reduced_hp against the y of the oracle's schur_solve: the forward error of a backward-stable
    solve, a small multiple of kappa eps (bar: the comparators' own)."""
    R = cpu_reference(oracle, name, MU0)
    cls = case_class(name, MU0)
    assert R["reps"]["oracle"]["fwd"] <= sh.bar("fwd", cls) and R["reps"]["oracle"]["eta"] <= sh.bar("eta", cls)
    y, yo = sh.to_f(R["ref"].y), R["ys"]["oracle"]
    assert np.linalg.norm(y - yo) <= sh.bar("fwd", cls) * sh.EPS * R["ref"].kappa * np.linalg.norm(y)


# ---- corruptions of a good result: each check fails when it should
def _good(R):
    return sh.comparator_outputs(R["ref"], R["ys"]["lapack"])


def _fails(R, out, cls):
    return sh.failed_checks(R["ref"].report(out), sh.STEP_METRICS, cls)


def _largest_forward_pivot(R):
    """the pivot whose column carries the most of the forward substitution (a reciprocal that scales nothing cannot show)"""
    L = np.linalg.cholesky(R["ref"].Sd)
    z = np.linalg.solve(L, R["ref"].rhs_d)
    return int(np.argmax(np.abs(z[:-1]) * np.linalg.norm(np.tril(L, -1), axis=0)[:-1]))


@pytest.mark.parametrize("name", NAMES)
def test_corrupted_reciprocals_fail(oracle, name):
    R = cpu_reference(oracle, name, MU0)
    ref = R["ref"]
    j = _largest_forward_pivot(R)
    bad = _fails(R, sh.comparator_outputs(ref, sh.textbook_solve(ref.Sd, ref.rhs_d, bad_pivot=j, bad_rel=1e-9)), case_class(name, MU0))
    print(name, "pivot", j, "reciprocal off by 1e-9:", bad)
    assert bad
    try:
        bad = _fails(R, sh.comparator_outputs(ref, sh.textbook_solve(ref.Sd, ref.rhs_d, rcp=lambda x: sh.rcp_newton(x, 0))), case_class(name, MU0))
    except np.linalg.LinAlgError as e:
        bad = [("chol_fail", str(e), 0)]  # (errors of 2^-26 in the columns: a later pivot comes out negative)
    print(name, "reciprocal from the estimate alone:", bad)
    assert bad
    # One Newton step on an estimate good to 2^-26 leaves 2^-52 = 2 eps in a reciprocal: what a rounded division leaves, twice.  No
    # bar made of double-precision solvers can tell the two apart, and these do not (the figures are printed; nothing to assert).
    rep = R["ref"].report(sh.comparator_outputs(ref, sh.textbook_solve(ref.Sd, ref.rhs_d, rcp=lambda x: sh.rcp_newton(x, 1))))
    print(name, f"reciprocal with one Newton step: eta={rep['eta']:.2f} fwd={rep['fwd']:.3g}", sh.failed_checks(rep, sh.STEP_METRICS, case_class(name, MU0)))


@pytest.mark.parametrize("name", NAMES)
def test_corrupted_assembly_fails(oracle, name):
    """One IMU entry scattered one column off; one prior column dropped: the step solves another system (eta), and the matrix is not
    the oracle's."""
    R = cpu_reference(oracle, name, MU0)
    ref, w = R["ref"], R["w"]
    vis, blocks, A, cmap = oracle_sources(oracle, w)
    Ho = oracle.linearize(w)["H"]

    def fails(H):
        rd = sh.reduced_double(H, ref.gd, ref.Cd, ref.z1d, MU0, ref.red["active"])
        try:
            return _fails(R, sh.comparator_outputs(ref, sh.lapack_solve(rd["S"], rd["rhs"])), case_class(name, MU0))
        except np.linalg.LinAlgError:
            return [("chol_fail", 1, 0)]  # (the wrong matrix is not even positive definite)

    f = next(f for f in range(10) if blocks[f].any())
    cols = sh.imu_columns(f)
    H = sh.to_f(sh.assemble_hp(vis, blocks, A, cmap, w.estimate_extrinsic, w.estimate_td))
    p, q = 8, 3  # (sb_f entry 2, pose_f entry 3) lands one column further right
    H[cols[p], cols[q] + 1] += blocks[f][p, q]
    H[cols[q] + 1, cols[p]] += blocks[f][p, q]
    H[cols[p], cols[q]] -= blocks[f][p, q]
    H[cols[q], cols[p]] -= blocks[f][p, q]
    assert np.abs(H - Ho).max() > 1e-13 * np.abs(Ho).max()
    bad = fails(H)
    print(name, "IMU entry one column off:", bad)
    assert bad
    if len(cmap):
        keep = np.arange(len(cmap)) != 7
        H = sh.to_f(sh.assemble_hp(vis, blocks, A[np.ix_(keep, keep)], cmap[keep], w.estimate_extrinsic, w.estimate_td))
        bad = fails(H)
        print(name, "prior column dropped:", bad)
        assert bad


@pytest.mark.parametrize("name,mu", RUNS, ids=[_rid(v) for v in RUNS])
def test_corrupted_mu_terms_fail(oracle, name, mu):
    """N^T H N without its mu term; G^T H N with the sign of its mu term flipped (the identities of solve_body: N^T H N = |z|^2 -
    mu |gauss_newton|^2 + N_c^T C N_c, G^T H N = -gamma^T rhs - mu gradient_ . gauss_newton + G_c^T C N_c)."""
    R = cpu_reference(oracle, name, mu)
    cls, m, unit = case_class(name, mu), R["ref"].model, sh.EPS * R["ref"].kappa
    # the size of what is corrupted, in the metric's unit, from the 50-digit model: where it is below the bar the comparators themselves
    # are no closer to the truth than the term is large, and no check can see it (the weak class at mu = 1e-8: kappa eps ~ 1e-5)
    size_nn = float(abs(mu * m["Q_GN_SQ"] / m["Q_NN"])) / unit
    size_gn = float(abs(2 * mu * m["Q_GRAD_GN"] / m["Q_GN"])) / unit
    print(name, mu, f"mu terms in units of eps kappa: Q_NN {size_nn:.3g} (bar {sh.bar('Q_NN', cls):.3g}), Q_GN {size_gn:.3g} (bar {sh.bar('Q_GN', cls):.3g})")
    if cls[0] != "weak":
        assert size_nn > 2 * sh.bar("Q_NN", cls) and size_gn > 2 * sh.bar("Q_GN", cls)
    out = _good(R)
    out["Q_NN"] += mu * out["Q_GN_SQ"]
    bad = _fails(R, out, cls)
    print(name, mu, "mu term missing from Q_NN:", bad)
    assert [b for b in bad if b[0] == "Q_NN"] or size_nn <= 2 * sh.bar("Q_NN", cls)
    out = _good(R)
    out["Q_GN"] += 2.0 * mu * out["Q_GRAD_GN"]
    bad = _fails(R, out, cls)
    print(name, mu, "mu term of Q_GN with the wrong sign:", bad)
    assert [b for b in bad if b[0] == "Q_GN"] or size_gn <= 2 * sh.bar("Q_GN", cls)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "imu_only"])
def test_corrupted_schur_sums_fail(oracle, name):
    R = cpu_reference(oracle, name, MU0)
    lin, N = R["lin"], R["w"].N
    k = int(np.argmin(np.abs(lin["W"]).sum(axis=1) + np.where(np.abs(lin["W"]).sum(axis=1) > 0, 0.0, np.inf)))  # the lightest landmark
    rep = sh.schur_report(sh.schur_double(lin["a"], lin["b"], lin["W"], MU0, [l for l in range(N) if l != k]), R["sch"])
    print(name, "landmark", k, "left out:", rep)
    assert [b for b in sh.failed_checks(rep, sh.SCHUR_METRICS, case_class(name, MU0)) if b[0] == "C"]
    good = sh.schur_double(lin["a"], lin["b"], lin["W"], MU0)
    a = lin["a"]
    s2 = (1.0 / (1.0 + np.sqrt(a))) ** 2
    einv = 1.0 / (s2 * a + MU0 * np.clip(s2 * a, sh.MIN_DIAG, sh.MAX_DIAG))  # 1 / e_l where s_l^2 / e_l belongs
    good["z1"] = (einv * lin["b"]) @ lin["W"]
    rep = sh.schur_report(good, R["sch"])
    print(name, "z1 without landmark scaling:", rep)
    assert [b for b in sh.failed_checks(rep, sh.SCHUR_METRICS, case_class(name, MU0)) if b[0] == "z1"]


# ------------------------------------------------------------------------------------------------------------------------
# GPU: one pass per route and mu on the device, through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------
_dev = dict(route=None, io={})


def schur_index(r, c):
    """where entry (r, c), r <= c, of the 80 x 80 accumulator sits in the 15 tiles of the exchange buffer (csrc/kernels_lin.h)"""
    t, u = r >> 4, c >> 4
    return (t * 5 - t * (t - 1) // 2 + (u - t)) * 256 + ((r & 15) >> 2) * 64 + ((r & 3) << 4) + (c & 15)


_SI = np.array([[schur_index(min(i, j), max(i, j)) for j in range(80)] for i in range(80)])


def device_io(eng, oracle, route, name, mu):
    """What the pass at `mu` over the resident batch of the route's cases read and wrote in the case's slot: one upload per route,
    one pass per (route, mu, slot)."""
    names = DEVICE_NAMES[route]
    if _dev["route"] != route:
        ws = [window(oracle, n) for n in names]
        eng.set_linw(route)
        eng.batch_reserve(len(ws), max(w.N for w in ws), max(w.M for w in ws))
        for s, w in enumerate(ws):
            eng.batch_upload(s, w)
        _dev["route"] = route
    key = (route, name, mu)
    if key not in _dev["io"]:
        io = eng.pass_io(len(names), names.index(name), window(oracle, name).N, mu)
        assert io["linw"] == (1 if route == LINW else 0), (route, io["linw"])
        full = io["schur"][_SI]
        io.update(C=full[:sh.KC, :sh.KC], z1=full[:sh.KC, 73], z2=full[:sh.KC, 74])
        _dev["io"][key] = io
    return _dev["io"][key]


@pytest.fixture(scope="module")
def dev(eng):
    yield eng
    eng.set_linw(1)


def device_H(io, route):
    """H_pp as the solve had it: the packed matrix k_sum left, or — behind k_linw — assembled in 50 digits from the three sources."""
    if route == ROLES:
        return sh.packed_lower(io["H"])
    vis = sh.packed_lower(io["H"][:sh.KC * (sh.KC + 1) // 2], sh.KC)
    return sh.assemble_hp(vis, io["imu_out"][:, :900].reshape(10, 30, 30), io["prior_A"], io["prior_cmap"], io["est_ex"], io["est_td"])


_dev_sch = {}


def device_schur_hp(io, route, name):
    """schur_hp of the run's own a, b, W at the first mu (z2 and the landmark scalars do not depend on mu)."""
    if (route, name) not in _dev_sch:
        _dev_sch[(route, name)] = sh.schur_hp(io["a"], io["b"], io["W"], MU0)
    return _dev_sch[(route, name)]


def device_outputs(io):
    out = {k: io[k] for k in ("scale_p", "diag_p", "grad_p", "gn_p", "uc_grad", "alpha")}
    out.update({k: io["q"][i] for i, k in enumerate(sh.Q_NAMES)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route,name,mu", DEVICE_RUNS, ids=[_rid(v) for v in DEVICE_RUNS])
def test_device_step_and_scalars(dev, oracle, route, name, mu):
    io0 = device_io(dev, oracle, route, name, MU0)
    io = device_io(dev, oracle, route, name, mu)
    assert io["chol_fail"] == 0 and io["mu"] == mu
    ref = sh.Reference(device_H(io, route), io["gp"], io["C"], io["z1"], mu, sh.active_columns(io["est_ex"], io["est_td"]),
                       device_schur_hp(io0, route, name))
    assert ref.cert < sh.CERTIFICATE
    cls = case_class(name, mu)
    rep = ref.report(device_outputs(io))
    print(_line(f"{_rid((route, name, mu))} device", ref, rep, cls))
    assert abs(io["grad_sq_total"] - float(ref.model["grad_sq_total"])) <= sh.bar("Q_GRAD_SQ", cls) * sh.EPS * float(ref.model["grad_sq_total"])
    # N = -scale y and gauss_newton_step_ = -diagonal_ y are two roundings of products with the same y
    un, gn, s, d = (sh.to_mp(io[k][:sh.KC]) for k in ("uc_gn", "gn_p", "scale_p", "diag_p"))
    for i in range(sh.KC):
        assert abs(un[i] * d[i] - gn[i] * s[i]) <= 2.01 * sh.EPS * abs(gn[i] * s[i]), i
    assert sh.failed_checks(rep, sh.STEP_METRICS, cls) == []


@pytest.mark.gpu
@pytest.mark.parametrize("route,name", DEVICE_CASES, ids=[_rid(v) for v in DEVICE_CASES])
def test_device_schur_sums(dev, oracle, route, name):
    io = device_io(dev, oracle, route, name, MU0)
    w = window(oracle, name)
    hp = device_schur_hp(io, route, name)
    rep = sh.schur_report(dict(C=io["C"], z1=io["z1"], z2=io["z2"], ls1=io["lm_sum"][1], ls2=io["lm_sum"][2]), hp)
    print(f"{_rid((route, name))} device schur: " + " ".join(f"{k}={rep[k]:.2f}" for k in sh.SCHUR_METRICS))
    assert np.array_equal(io["C"], io["C"].T)
    assert io["lm_sum"][4] == (np.abs(io["b"]).max() if w.N else 0.0)
    lam2 = float(sum(sh.to_mp(w.inv_depth) ** 2)) if w.N else 0.0
    assert abs(io["lm_sum"][3] - lam2) <= sh.bar("ls1", case_class(name, MU0)) * sh.EPS * lam2
    assert sh.failed_checks(rep, sh.SCHUR_METRICS, case_class(name, MU0)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("route,name", DEVICE_CASES, ids=[_rid(v) for v in DEVICE_CASES])
def test_device_exact_properties(dev, oracle, route, name):
    io = device_io(dev, oracle, route, name, MU0)
    w = window(oracle, name)
    act = sh.active_columns(w.estimate_extrinsic, w.estimate_td)
    assert (io["est_ex"], io["est_td"]) == (w.estimate_extrinsic, w.estimate_td)
    for k in ("gn_p", "grad_p"):
        assert np.all(io[k][~act] == 0.0), k
    for k in ("uc_grad", "uc_gn"):
        assert np.all(io[k][:sh.KC][~act[:sh.KC]] == 0.0) and np.all(io[k][sh.KC:] == 0.0), k
    assert io["chol_fail"] == 0 and io["mu"] == MU0
    assert np.all(io["W"][:, ~act[:sh.KC]] == 0.0)
    # the sources of the assembly: zeros for a skipped factor, the prior's map; k_lin leaves whole symmetric blocks (k_linw only the
    # entries whose tangent row is not above their column: what assemble_hp reads)
    blocks = io["imu_out"][:, :900].reshape(10, 30, 30)
    for f in range(10):
        assert route == LINW or np.array_equal(blocks[f], blocks[f].T), f
        assert blocks[f].any() == (not w.imu[f].sum_dt > 10.0), f
    if w.prior is not None and w.prior.valid:
        assert io["prior_n"] == w.prior.n and np.array_equal(io["prior_cmap"], sh.prior_column_map(w.prior))
        assert np.array_equal(io["prior_A"], io["prior_A"].T)
    else:
        assert io["prior_n"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("route", [ROLES, LINW], ids=["roles", "linw"])
def test_device_no_attempt_at_mu_one(dev, oracle, route):
    """ComputeGaussNewtonStep is `while (mu < max_mu)`: at mu = 1 the pass reports the failure and leaves mu alone."""
    device_io(dev, oracle, route, "n64", MU0)
    io = dev.pass_io(len(DEVICE_NAMES[route]), DEVICE_NAMES[route].index("n64"), window(oracle, "n64").N, 1.0)
    assert io["chol_fail"] == 1 and io["mu"] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("route", [ROLES, LINW], ids=["roles", "linw"])
def test_device_two_runs_give_the_same_bits(dev, oracle, route):
    names = DEVICE_NAMES[route]
    for name in names:
        a = device_io(dev, oracle, route, name, MU0)
        b = dev.pass_io(len(names), names.index(name), window(oracle, name).N, MU0)
        for k in ("schur", "gp", "lm_sum", "scale_p", "diag_p", "grad_p", "gn_p", "uc_grad", "uc_gn", "q"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert (a["alpha"], a["grad_sq_total"], a["x_cost"]) == (b["alpha"], b["grad_sq_total"], b["x_cost"]), name
