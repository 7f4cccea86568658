"""lfvio_pnp (k_pnp) against a 50-digit reference and against the numpy restatement.

The fixtures tests/golden/pnp_hp.npz hold PnP cases and the results of the mpmath side of tests/pnp_ref.py rounded to
double; tests/golden/gen_pnp_hp.py writes them.  After its 15 Gauss-Newton steps the solver's three candidates agree far
below double precision on every fixture (the file's `spread`), so which of them wins is decided by rounding: the tests
hold R, T and the winning error, never `chosen`.  A result is compared with whichever of the reference's three candidates
it is closest to, among those whose 50-digit error exceeds the best one by no more than the bar of `err`.  Metrics:

  R     largest |difference| of an entry of compute_pose's R, in units of eps
  T     largest |difference| of an entry of T, in units of eps x the largest |x_w| of the case
  err   |err[chosen] - the candidate's error|, relative, in units of eps

BARS.  bar = 16 x the worst value the numpy restatement (pnp_ref.compute_pose) reaches against the same fixtures, per metric
and regime, floor 2 (eps units), as tests/test_two_view.py has it.  REF below is that measurement;
test_restatement_holds_its_record re-measures it on the CPU and holds it to the table.  Against the restatement itself
(batches): bar + REF, the largest over the regimes of ordinary size.

worst restatement / bar / worst device (MI355X), per regime (4 cases each)
  regime       R                     T                     err
  clean        2e+02/3.2e+03/not measured     5.6e+02/8.96e+03/not measured  2e+02/3.2e+03/not measured
  noisy        1.6e+02/2.56e+03/not measured  3.5e+03/5.6e+04/not measured   4.9e+02/7.84e+03/not measured
  zneg         79/1.26e+03/not measured       90/1.44e+03/not measured       30/480/not measured
  zpos         57/912/not measured            1.8e+02/2.88e+03/not measured  97/1.55e+03/not measured
  annulus      3.1e+05/4.96e+06/not measured  4.1e+06/6.56e+07/not measured  4.5e+05/7.2e+06/not measured
  minimal      4.8e+02/7.68e+03/not measured  7.1e+02/1.14e+04/not measured  1.3e+03/2.08e+04/not measured
  large        1.8e+04/2.88e+05/not measured  1.4e+05/2.24e+06/not measured  2.9e+03/4.64e+04/not measured
  depthspread  2e+02/3.2e+03/not measured     5.8e+02/9.28e+03/not measured  1.6e+02/2.56e+03/not measured
"""
import ctypes as C
import os

import numpy as np
import pytest

import pnp_ref as pr
from golden import gen_pnp_hp as gen

EPS = 2.0 ** -52
FACTOR = 16.0
FLOOR = 2.0
METRICS = ("R", "T", "err")
REGIMES = ("clean", "noisy", "zneg", "zpos", "annulus", "minimal", "large", "depthspread")

# worst value of the numpy restatement against the 50-digit fixtures, per regime (rounded up to two digits)
REF = {
    "clean": dict(R=2e+02, T=5.6e+02, err=2e+02),
    "noisy": dict(R=1.6e+02, T=3.5e+03, err=4.9e+02),
    "zneg": dict(R=79, T=90, err=30),
    "zpos": dict(R=57, T=1.8e+02, err=97),
    "annulus": dict(R=3.1e+05, T=4.1e+06, err=4.5e+05),
    "minimal": dict(R=4.8e+02, T=7.1e+02, err=1.3e+03),
    "large": dict(R=1.8e+04, T=1.4e+05, err=2.9e+03),
    "depthspread": dict(R=2e+02, T=5.8e+02, err=1.6e+02),
}


def bar(regime, metric):
    return max(FACTOR * REF[regime][metric], FLOOR)


def loose_bar(metric, regimes=("clean", "noisy", "zneg", "zpos", "annulus", "depthspread")):
    """Against the restatement: its own error on top of the bar."""
    return max(bar(r, metric) + REF[r][metric] for r in regimes)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "pnp_hp.npz"))
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["names"]}


def compare(got, R_all, T_all, err, scale, err_bar, tag, bars):
    """`got` (a dict of Engine.pnp / pnp_ref.compute_pose) against the reference's candidates.  Returns {metric: value}."""
    assert got["status"] == 0, tag
    best = float(np.min(err))
    ok = [c for c in range(3) if float(err[c]) - best <= err_bar * EPS * best]
    dist = lambda c: max(np.abs(np.asarray(got["R"], float) - R_all[c]).max(), np.abs(np.asarray(got["T"], float) - T_all[c]).max() / scale)
    c = min(ok, key=dist)
    m = dict(R=float(np.abs(np.asarray(got["R"], float) - R_all[c]).max() / EPS), T=float(np.abs(np.asarray(got["T"], float) - T_all[c]).max() / (EPS * scale)),
             err=float(abs(float(got["err"][got["chosen"]]) - float(err[c])) / (EPS * float(err[c]))))
    if bars is not None:
        bad = [f"{tag} {k}: {v:.3g} > bar {bars[k]:.3g}" for k, v in m.items() if not v <= bars[k]]
        assert not bad, "\n".join(bad)
    return m


def measure(fn, fx, use_bars):
    worst = {r: dict.fromkeys(METRICS, 0.0) for r in REGIMES}
    for name, f in fx.items():
        regime = name.rsplit("_", 1)[0]
        got = fn(f["pw"], f["us"])
        m = compare(got, f["R_all"], f["T_all"], f["err"], float(np.abs(f["pw"]).max()), bar(regime, "err"), name,
                    {k: bar(regime, k) for k in METRICS} if use_bars else None)
        print(f"  {name:14s} n {len(f['pw']):5d} " + " ".join(f"{k} {v:9.3g}" for k, v in m.items()))
        for k, v in m.items():
            worst[regime][k] = max(worst[regime][k], v)
    return worst


def show(worst):
    for r in REGIMES:
        print(f'    "{r}": dict(' + ", ".join(f"{k}={worst[r][k]:.2g}" for k in METRICS) + "),")


def restatement(pw, us):
    with np.errstate(all="ignore"):
        return pr.compute_pose(pw, us)


def test_fixture_regimes(fixtures):
    """CPU: the file holds the regimes and sizes it is meant to: at least 4 cases each, the sign conditions of zneg / zpos,
    bearings on both sides of z = 0 in `annulus`, the sizes of `minimal` and `large`, candidates that agree."""
    for r in REGIMES:
        assert sum(n.rsplit("_", 1)[0] == r for n in fixtures) >= 4, r
    for n, f in fixtures.items():
        r = n.rsplit("_", 1)[0]
        z = f["us"][:, 2]
        assert np.all(z != 0) and f["spread"].max() < 1e-18, n
        if r == "zneg":
            assert np.all(z < 0)
        if r == "zpos":
            assert np.all(z > 0)
        if r == "annulus":
            assert np.any(z < 0) and np.any(z > 0) and np.abs(z).min() < 0.01
    assert sorted(len(fixtures[f"minimal_{c}"]["pw"]) for c in range(4)) == [6, 7, 8, 10]
    assert sorted(len(fixtures[f"large_{c}"]["pw"]) for c in range(4)) == [1000, 1000, 4096, 4096]
    d = np.concatenate([np.linalg.norm(fixtures[f"depthspread_{c}"]["pw"] @ fixtures[f"depthspread_{c}"]["R_true"].T + fixtures[f"depthspread_{c}"]["t_true"], axis=1)
                        for c in range(4)])
    assert d.min() < 0.5 and d.max() > 40.0


def test_restatement_holds_its_record(fixtures):
    """CPU: the numpy restatement against the 50-digit fixtures is what REF says (REF is rounded up to two digits), on every
    metric and regime."""
    worst = measure(restatement, fixtures, False)
    show(worst)
    for r in REGIMES:
        for k in METRICS:
            assert worst[r][k] <= REF[r][k] * (1 + 1e-9), (r, k, worst[r][k], REF[r][k])
            assert worst[r][k] >= 0.5 * REF[r][k] or REF[r][k] < 1e-3, f"REF[{r}][{k}] = {REF[r][k]} is stale: measured {worst[r][k]}"


def test_fixtures_are_the_generators(fixtures):
    """CPU: one case of the file re-derived by the 50-digit side, bit for bit (the file is what the generator writes)."""
    f = fixtures["minimal_1"]
    rec = gen.hp_case(f["pw"], f["us"])
    for k in ("R_all", "T_all", "err", "spread"):
        assert np.array_equal(np.asarray(rec[k]), f[k]), k
    assert rec["chosen"] == int(f["chosen"])


def degenerate_cases():
    """(pw, us) with status 1: one bearing with z == 0; exactly coplanar points (the plane z = 2 of the world frame: the
    moment matrix has an exactly zero row, its third control point coincides with the first and CC is singular)."""
    a = gen.make_case(71, 40)
    us = a["us"].copy()
    us[17, 2] = 0.0
    b = gen.make_case(72, 50)
    pw = b["pw"].copy()
    pw[:, 2] = 2.0
    return [(a["pw"], us), (pw, b["us"])]


def test_restatement_reports_the_degenerate_inputs():
    """CPU: both kinds of degenerate input give status 1 in the restatement (the device's deviation 1, restated)."""
    for pw, us in degenerate_cases():
        assert restatement(pw, us)["status"] == 1


def test_colpiv_solve_drops_a_dependent_column():
    """CPU: the restated colPivHouseholderQr().solve — full rank: the least-squares solution; a column 1e-20 x the others (below
    Eigen's threshold, eps x the largest column norm): the factorization ends there and the dropped component is exactly 0.
    (A column that merely repeats another leaves a remainder of a few eps, right at the threshold: rounding decides, in Eigen too.)"""
    rng = np.random.default_rng(5)
    A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
    x = pr.colpiv_solve(A, b, pr.F64)
    assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=0, atol=1e-13)
    A[:, 2] *= 1e-20
    x = pr.colpiv_solve(A, b, pr.F64)
    assert x[2] == 0.0 and np.all(x[[0, 1, 3]] != 0.0)
    assert np.allclose(x[[0, 1, 3]], np.linalg.lstsq(A[:, [0, 1, 3]], b, rcond=None)[0], rtol=0, atol=1e-13)


def device(eng):
    return lambda pw, us: eng.pnp([0, len(pw)], pw, us)[0]


@pytest.mark.gpu
def test_fixtures_every_metric_per_regime(eng, fixtures):
    """Test 5: every metric on the fixtures, per regime, the device held to 16 x the restatement's own error."""
    worst = measure(device(eng), fixtures, True)
    show(worst)


def batch(F, seed=100):
    """F frames of 6 .. 300 correspondences from gen.make_case, as a CSR."""
    rng = np.random.default_rng(seed)
    cases = [gen.make_case(seed + 1 + f, int(rng.integers(6, 301)), noise_px=0.3 if f % 3 else 1.0) for f in range(F)]
    off = np.concatenate([[0], np.cumsum([len(c["pw"]) for c in cases])]).astype(np.int32)
    return off, np.concatenate([c["pw"] for c in cases]), np.concatenate([c["us"] for c in cases])


def same_bits(a, b):
    return a["status"] == b["status"] and a["chosen"] == b["chosen"] and all(np.array_equal(a[k], b[k]) for k in ("R", "T", "err"))


@pytest.mark.gpu
def test_a_repeated_call_returns_the_same_bits(eng, fixtures):
    """Test 6a."""
    for name in ("noisy_0", "minimal_0", "large_1"):
        f = fixtures[name]
        a, b = device(eng)(f["pw"], f["us"]), device(eng)(f["pw"], f["us"])
        assert a["status"] == 0 and same_bits(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 7, 128])
def test_a_batch_returns_the_bits_of_single_calls(eng, F):
    """Test 6b: F frames in one call against F calls of one frame; and against the restatement, bar + REF."""
    off, pw, us = batch(F)
    res = eng.pnp(off, pw, us)
    assert len(res) == F
    for f in range(F):
        p, u = pw[off[f]:off[f + 1]], us[off[f]:off[f + 1]]
        assert same_bits(res[f], device(eng)(p, u)), f
        if off[f + 1] - off[f] >= 30:
            r = restatement(p, u)
            lb = {k: loose_bar(k) for k in METRICS}
            compare(res[f], r["R_all"], r["T_all"], r["err"], float(np.abs(p).max()), lb["err"], f"F={F} frame {f}", lb)


def filled(F):
    from lfvio import abi

    out = (abi.PnpOutC * F)()
    for f in range(F):
        out[f].status, out[f].chosen = 70 + f, 80 + f
        for k in range(9):
            out[f].R[k] = 1.5 + k + f
        for k in range(3):
            out[f].T[k], out[f].err[k] = 2.5 + k + f, 3.5 + k + f
    return out


@pytest.mark.gpu
def test_a_degenerate_frame_in_a_batch(eng):
    """Test 6c: a status-1 frame in the middle of a batch leaves its outputs untouched (status apart) and its neighbours'
    bits unchanged; both kinds of degenerate input."""
    off, pw, us = batch(5, seed=300)
    clean = eng.pnp(off, pw, us)
    assert all(r["status"] == 0 for r in clean)
    for dpw, dus in degenerate_cases():
        off2 = np.concatenate([off[:3], off[2:] + len(dpw)]).astype(np.int32)
        pw2, us2 = np.concatenate([pw[:off[2]], dpw, pw[off[2]:]]), np.concatenate([us[:off[2]], dus, us[off[2]:]])
        out = filled(6)
        before = bytes(out[2])[8:]
        res = eng.pnp(off2, pw2, us2, out=out)
        assert res[2]["status"] == 1 and bytes(out[2])[8:] == before and out[2].chosen == 82
        for f, g in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4)):
            assert same_bits(res[f], clean[g]), (f, g)


@pytest.mark.gpu
def test_argument_errors_leave_the_outputs_alone(eng):
    """Test 6d: every LFVIO_ERR_ARG case."""
    from lfvio import abi

    off, pw, us = batch(3, seed=400)
    pw, us = np.tile(pw, (20, 1)), np.tile(us, (20, 1))  # (long enough for every CSR below)
    big = gen.make_case(9, 4097)
    cases = {
        "5 correspondences": ([0, 5], pw[:5], us[:5]),
        "5 in the middle": ([0, off[1], off[1] + 5, off[1] + 5 + 40], pw[:off[1] + 45], us[:off[1] + 45]),
        "4097 correspondences": ([0, 4097], big["pw"], big["us"]),
        "not ascending": ([0, 40, 30, 80], pw[:80], us[:80]),
        "offset[0] != 0": ([1, 41], pw[:41], us[:41]),
        "129 frames": (np.arange(130) * 6, np.tile(pw[:6], (129, 1)), np.tile(us[:6], (129, 1))),
    }
    for tag, (o, p, u) in cases.items():
        out = filled(max(len(o) - 1, 1))
        before = bytes(out)
        rc, _ = eng.pnp(o, p, u, out=out, check=False)
        assert rc == -1 and bytes(out) == before, tag
    out = filled(1)
    before = bytes(out)
    pin = abi.PnpInC()
    pin.num_frames = 0
    assert eng.lib.lfvio_pnp(eng.ctx, C.byref(pin), out) == -1  # F = 0
    pin.num_frames = 1
    assert eng.lib.lfvio_pnp(eng.ctx, C.byref(pin), out) == -1  # null arrays
    assert eng.lib.lfvio_pnp(eng.ctx, None, out) == -1 and bytes(out) == before
    o32 = np.array([0, 40], np.int32)
    pin.offset, pin.point_w, pin.bearing = o32.ctypes.data_as(C.POINTER(C.c_int)), pw.ctypes.data_as(C.POINTER(C.c_double)), us.ctypes.data_as(C.POINTER(C.c_double))
    assert eng.lib.lfvio_pnp(eng.ctx, C.byref(pin), None) == -1
    assert eng.pnp([0, 40], pw[:40], us[:40])[0]["status"] == 0  # the context is still good
