"""lfvio_two_view (k_tv_hyp, k_tv_fit) against a 50-digit reference and against the numpy restatement.

The fixtures tests/golden/twoview_hp.npz hold two-view cases and the results of the mpmath side of tests/twoview_ref.py
rounded to double; tests/golden/gen_twoview_hp.py writes them.  Metrics, each in the unit that its error scales with:

  E_all     every hypothesis' E, Frobenius-normalised, up to sign: distance in units of
            eps (sigma_1/sigma_8 of its 8 x 9 system + sigma_1/(sigma_2 - sigma_3) of its E_0)
  score     every hypothesis' score, relative (float accumulator: a difference is 0 or >= 6e-8)
  E         the refit E, the same two terms of the n x 9 inlier system and its E_0
  cand      the candidate set {R1, R2} x {+-t} as a set, worst angle, in units of eps sigma_1/sigma_2 of the refit E_0
  R_rel     angle to the reference's R_rel, same unit
  exact     best_sample, num_inliers, the mask, the four front counts, the chosen candidate — under the conditions
            C1 (the winner's score exceeds the runner-up's of another sample set by > 1e-4 relative), C2 (no residual
            of the winner or the refit within 1e-6 thr of thr), C3 (|ratio1 - ratio2| >= 2 / N), all judged on the
            numpy restatement; a case that breaks one drops the exact comparisons only, at most 10 % of a test's cases

BARS.  bar = 16 x the worst value the numpy restatement (twoview_ref.two_view) reaches against the same fixtures, per
metric and regime, floor 2 (eps units) / 2 eps (score).  REF below is that measurement; test_restatement_holds_its_record
re-measures it on the CPU and holds it to the table.  Against the restatement itself (sizes, ties): bar + REF, as
test_feature_hp does for its oracle; sizes below 30 matches take the regime `minimal`, the others the largest bar of the
six regimes of ordinary size.

worst restatement / bar / worst device (MI355X), per regime (4 cases each; minimal: N = 8, 9, 10, 12)
  regime     E_all                   score                   E                       cand                    R_rel
  clean      0.46/7.36/0.44          0/4.44e-16/0            0.31/4.96/0.078         43/688/14               35/560/3.7
  noisy      0.55/8.8/0.44           0/4.44e-16/0            0.75/12/0.084           32/512/7.1              30/480/2.4
  outliers   0.42/6.72/0.45          0/4.44e-16/0            0.23/3.68/0.14          31/496/5.1              2.7/43.2/5.1
  smallbase  0.38/6.08/0.45          0/4.44e-16/0            0.84/13.4/0.29          700/11200/220            3.6/57.6/2.5
  zneg       0.46/7.36/0.41          0/4.44e-16/0            0.087/2/0.041           11/176/5.9              3.9/62.4/1.7
  zpos       0.76/12.2/0.3           0/4.44e-16/0            0.31/4.96/0.074         88/1408/11              4/64/3.4
  minimal    0.46/7.36/0.19          0/4.44e-16/0            0.46/7.36/0.16          320/5120/200            24/384/5.8
  (E_all, E, cand, R_rel in the eps units above; score relative: restatement, device and the 50-digit side agree bit for bit
  on every hypothesis.  Sizes N x S against the restatement: worst E_all 2.61, E 0.53, cand 1.4e3, R_rel 18.5; of the 55
  combinations 3 give no model on both sides, none of the other 52 breaks C1 - C3.  Pure rotation: the device's angle to the
  true rotation equals the restatement's to three digits, 5.5e-4 .. 9.9e-4 rad at 0.3 px.)
"""
import os

import numpy as np
import pytest

import twoview_ref as tv
from golden import gen_twoview_hp as gen

EPS = 2.0 ** -52
FACTOR = 16.0
FLOOR = {"E_all": 2.0, "score": 2 * EPS, "E": 2.0, "cand": 2.0, "R_rel": 2.0}
METRICS = ("E_all", "score", "E", "cand", "R_rel")
REGIMES = ("clean", "noisy", "outliers", "smallbase", "zneg", "zpos", "minimal")

# worst value of the numpy restatement against the 50-digit fixtures, per regime (rounded up to two digits)
REF = {
    "clean": dict(E_all=0.46, score=0, E=0.31, cand=43, R_rel=35),
    "noisy": dict(E_all=0.55, score=0, E=0.75, cand=32, R_rel=30),
    "outliers": dict(E_all=0.42, score=0, E=0.23, cand=31, R_rel=2.7),
    "smallbase": dict(E_all=0.38, score=0, E=0.84, cand=7e+02, R_rel=3.6),
    "zneg": dict(E_all=0.46, score=0, E=0.087, cand=11, R_rel=3.9),
    "zpos": dict(E_all=0.76, score=0, E=0.31, cand=88, R_rel=4),
    "minimal": dict(E_all=0.46, score=0, E=0.46, cand=3.2e+02, R_rel=24),
}


def bar(regime, metric):
    return max(FACTOR * REF[regime][metric], FLOOR[metric])


def loose_bar(N, metric):
    """Against the restatement: its own error on top of the bar."""
    regs = ("minimal",) if N < 30 else REGIMES[:6]
    return max(bar(r, metric) + REF[r][metric] for r in regs)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "twoview_hp.npz"))
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["names"]}


def conditions(r):
    """C1 - C3 on a result of the restatement."""
    return r["status"] == 0 and r["c1_gap"] > 1e-4 and r["c2_margin"] > 1e-6 and r["c3_gap"] >= 2.0 - 1e-9


def compare(got, ref, cond_all, cond_refit, rank2, exact, tag, bars):
    """Every metric of `got` (Engine.two_view / twoview_ref.two_view) against `ref` (a fixture or the restatement).
    Returns {metric: value}; asserts the bars (a dict) where given and the exact part where `exact`."""
    S = len(ref["E_all"])
    m = {}
    m["E_all"] = max(tv.e_distance(got["E_all"][k], ref["E_all"][k]) / (EPS * (cond_all[k][0] + cond_all[k][1])) for k in range(S))
    gs, rs = np.asarray(got["score_all"], np.float64), np.asarray(ref["score_all"], np.float64)
    assert np.array_equal(gs[rs == 0], rs[rs == 0]), f"{tag}: a hypothesis that scores 0 in the reference"
    m["score"] = float(np.max(np.abs(gs - rs)[rs > 0] / rs[rs > 0])) if np.any(rs > 0) else 0.0
    assert got["status"] == 0, tag
    same_fit = int(got["best_sample"]) == int(ref["best_sample"]) or np.array_equal(np.sort(got["samples"][int(got["best_sample"])]), np.sort(got["samples"][int(ref["best_sample"])]))
    if exact or same_fit:
        m["E"] = tv.e_distance(got["E"], ref["E"]) / (EPS * (cond_refit[0] + cond_refit[1]))
        ang, front = tv.candidate_distance(got["R_cand"], got["t_cand"], got["front"], ref["R_cand"], ref["t_cand"], ref["front"])
        m["cand"] = ang / (EPS * rank2)
        m["R_rel"] = tv.rot_angle(got["R_rel"], ref["R_rel"]) / (EPS * rank2)
    if exact:
        N = len(ref["mask"])
        assert int(got["best_sample"]) == int(ref["best_sample"]), tag
        assert int(got["num_inliers"]) == int(ref["num_inliers"]) and np.array_equal(got["mask"], ref["mask"]), tag
        rf = np.asarray(ref["front"])
        rf = rf.astype(np.float64) / N if np.issubdtype(rf.dtype, np.integer) else rf  # the fixtures hold counts
        assert np.array_equal(np.rint(front * N), np.rint(rf * N)), f"{tag}: front {front * N} != {rf * N}"
    if bars is not None:
        bad = [f"{tag} {k}: {v:.3g} > bar {bars[k]:.3g}" for k, v in m.items() if not v <= bars[k]]
        assert not bad, "\n".join(bad)
    return m


def run_fixture(fn, fx, name, use_bars=True):
    regime = name.rsplit("_", 1)[0]
    f = fx[name]
    got = fn(f["bl"], f["br"], f["samples"])
    got["samples"] = f["samples"]
    r = tv.two_view(f["bl"], f["br"], f["samples"])
    ok = conditions(r) and float(f["c2_margin"]) > 1e-6
    m = compare(got, f, f["cond_all"], f["cond_refit"], float(f["rank2"]), ok, name, {k: bar(regime, k) for k in METRICS} if use_bars else None)
    return regime, ok, m


def measure(fn, fx, use_bars):
    worst, dropped = {r: dict.fromkeys(METRICS, 0.0) for r in REGIMES}, []
    for name in fx:
        regime, ok, m = run_fixture(fn, fx, name, use_bars)
        if not ok:
            dropped.append(name)
        for k, v in m.items():
            worst[regime][k] = max(worst[regime][k], v)
    assert len(dropped) <= 0.1 * len(fx), f"more than 10 % of the cases break C1 - C3: {dropped}"
    return worst


def show(worst):
    for r in REGIMES:
        print(f'    "{r}": dict(' + ", ".join(f"{k}={worst[r][k]:.2g}" for k in METRICS) + "),")


def test_restatement_holds_its_record(fixtures):
    """CPU: the numpy restatement against the 50-digit fixtures is what REF says (within rounding of the table: REF is
    rounded up to two digits), on every metric and regime; the exact part holds on the restatement; the generator's cases
    stay inside the 10 % that may break C1 - C3."""
    worst = measure(lambda bl, br, s: tv.two_view(bl, br, s), fixtures, False)
    show(worst)
    for r in REGIMES:
        for k in METRICS:
            assert worst[r][k] <= REF[r][k] * (1 + 1e-9), (r, k, worst[r][k], REF[r][k])
            assert worst[r][k] >= 0.5 * REF[r][k] or REF[r][k] < 1e-3, f"REF[{r}][{k}] = {REF[r][k]} is stale: measured {worst[r][k]}"


def test_fixtures_are_the_generators(fixtures):
    """CPU: one case of the file re-derived by the 50-digit side, bit for bit (the file is what the generator writes)."""
    f = fixtures["minimal_1"]
    rec = gen.hp_case(f["bl"], f["br"], f["samples"])
    for k in ("E_all", "score_all", "E", "mask", "R_cand", "t_cand", "front", "R_rel"):
        assert np.array_equal(np.asarray(rec[k]), f[k]), k
    assert rec["best_sample"] == int(f["best_sample"]) and rec["num_inliers"] == int(f["num_inliers"])


def device(eng):
    return lambda bl, br, s: eng.two_view(bl, br, s, all_hypotheses=True)


@pytest.mark.gpu
def test_fixtures_every_metric_per_regime(eng, fixtures):
    """Test 1: every metric on the fixtures, per regime, the device held to 16 x the restatement's own error."""
    worst = measure(device(eng), fixtures, True)
    show(worst)


SIZES_N = (8, 9, 63, 64, 65, 150, 255, 256, 257, 1000, 4096)
SIZES_S = (1, 7, 100, 101, 1024)


@pytest.mark.gpu
def test_sizes_against_the_restatement(eng):
    """Test 2: N x S over the edges of the kernels' tiles (64 lanes, 256 threads, chunks of 1024 matches, the 1024
    samples of the selection), sample sets sorted (gen.make_samples)."""
    dropped, worst, total = [], dict.fromkeys(METRICS, 0.0), 0
    for i, N in enumerate(SIZES_N):
        c = gen.make_case(1000 + i, N, noise_px=0.1 if N < 30 else 0.3, outliers=0.0 if N < 30 else 0.1)
        for j, S in enumerate(SIZES_S):
            s = gen.make_samples(2000 + 10 * i + j, N, S, sort=True)
            r = tv.two_view(c["bl"], c["br"], s)
            if r["status"] != 0:  # (too few matches for the threshold: no model on either side)
                d = eng.two_view(c["bl"], c["br"], s)
                assert (d["status"], d["best_sample"], d["num_inliers"]) == (1, r["best_sample"], r["num_inliers"]), (N, S)
                continue
            total += 1
            ok = conditions(r)
            if not ok:
                dropped.append((N, S))
            d = eng.two_view(c["bl"], c["br"], s, all_hypotheses=True)
            d["samples"] = s
            m = compare(d, r, r["cond_all"], r["cond_refit"], r["rank2"], ok, f"N={N} S={S}", {k: loose_bar(N, k) for k in METRICS})
            for k, v in m.items():
                worst[k] = max(worst[k], v)
    print("sizes: worst", {k: f"{v:.3g}" for k, v in worst.items()}, "dropped", dropped, "of", total)
    assert total >= 50 and len(dropped) <= 0.1 * total, dropped


@pytest.mark.gpu
def test_first_of_equal_scores_wins(eng):
    """Test 3: the winning sample set repeated at indices 3 and 70 — best_sample == 3 (strict <, :197-202)."""
    c = gen.make_case(31, 150, noise_px=0.3, outliers=0.2)
    s = gen.make_samples(32, 150, 100)
    r = tv.two_view(c["bl"], c["br"], s)
    win = s[r["best_sample"]].copy()
    others = [k for k in range(100) if k != r["best_sample"]]
    s2 = s.copy()
    s2[3], s2[70] = win, win
    if r["best_sample"] not in (3, 70):
        s2[r["best_sample"]] = s[others[5]]
    r2 = tv.two_view(c["bl"], c["br"], s2)
    assert r2["best_sample"] == 3 and conditions(r2)
    d = eng.two_view(c["bl"], c["br"], s2, all_hypotheses=True)
    assert d["best_sample"] == 3 and d["score_all"][3] == d["score_all"][70] and np.array_equal(d["E_all"][3], d["E_all"][70])
    assert d["best_score"] == float(d["score_all"][3]) and np.array_equal(d["mask"], r2["mask"])


def no_model_cases():
    """Seeds of two UNRELATED bearing clouds (N = 40, S = 1 .. 3) on which the restatement reports (a) every hypothesis
    scoring exactly 0 and (b) a winner with a positive score and fewer than 8 inliers; two of each kind."""
    out = {"a": [], "b": []}
    for seed in range(400):
        rng = np.random.default_rng([seed, 77])
        bl, br = gen.annulus(rng, 40, (40.0, 120.0)), gen.annulus(rng, 40, (40.0, 120.0))
        s = gen.make_samples(seed, 40, 1 + seed % 3)
        r = tv.two_view(bl, br, s)
        kind = "a" if r["best_sample"] < 0 else "b" if r["status"] == 1 else None
        if kind and len(out[kind]) < 2:
            out[kind].append((bl, br, s, r))
        if len(out["a"]) == 2 and len(out["b"]) == 2:
            break
    return out


@pytest.mark.gpu
def test_no_model(eng):
    """Test 4: status 1 both ways, and everything but status, best_sample, num_inliers and best_score left as it was."""
    from lfvio import abi

    cases = no_model_cases()
    assert len(cases["a"]) == 2 and len(cases["b"]) == 2
    for kind in ("a", "b"):
        for bl, br, s, r in cases[kind]:
            out = abi.TwoViewOutC()
            for k in range(9):
                out.E[k], out.R_cand[0][k], out.R_cand[1][k], out.R_rel[k] = 1.5 + k, 2.5 + k, 3.5 + k, 4.5 + k
            for k in range(4):
                out.front[k] = 7.0 + k
            for k in range(3):
                out.t_cand[k] = 9.0 + k
            before = bytes(out)[24:]
            mask = np.full(40, 5, np.uint8)
            d = eng.two_view(bl, br, s, all_hypotheses=True, out=out, inlier=mask)
            assert d["status"] == 1 and d["rc"] == 0
            assert d["best_sample"] == r["best_sample"] and d["num_inliers"] == r["num_inliers"], kind
            assert np.array_equal(d["score_all"], r["score_all"])
            if kind == "a":
                assert d["best_sample"] == -1 and d["num_inliers"] == 0 and d["best_score"] == 0.0 and not d["score_all"].any()
            else:
                assert d["best_sample"] >= 0 and 0 < d["num_inliers"] < 8 and d["best_score"] == float(r["score_all"][d["best_sample"]]) > 0
            assert bytes(out)[24:] == before and np.all(mask == 5)


PURE_ROTATION = [(41, 60, 2.0), (42, 150, 5.0), (43, 300, 9.0), (44, 100, 0.7)]


def pure_rotation_case(seed, N, deg):
    c = gen.make_case(seed, N, noise_px=0.3, outliers=0.0, rot_deg=deg, baseline=0.0)
    return c, gen.make_samples(seed + 100, N, 100)


@pytest.mark.gpu
def test_pure_rotation(eng):
    """Test 5: zero baseline — E is not determined, only R_rel is held, against the TRUE relative rotation; bar = 16 x the
    restatement's own error on the same case."""
    for seed, N, deg in PURE_ROTATION:
        c, s = pure_rotation_case(seed, N, deg)
        r = tv.two_view(c["bl"], c["br"], s)
        d = eng.two_view(c["bl"], c["br"], s)
        assert r["status"] == 0 and d["status"] == 0
        er, ed = tv.rot_angle(r["R_rel"], c["R"].T), tv.rot_angle(d["R_rel"], c["R"].T)
        print(f"pure rotation N={N} {deg} deg: restatement {er:.3e} rad, device {ed:.3e} rad")
        assert ed <= 16.0 * er, (seed, ed, er)


@pytest.mark.gpu
def test_argument_errors_and_regrowth(eng):
    """Test 6a: LFVIO_ERR_ARG leaves the outputs alone; a second call with a larger N regrows the staging block."""
    import ctypes as C

    from lfvio import abi

    c = gen.make_case(51, 40)
    s = gen.make_samples(52, 40, 5)
    out = abi.TwoViewOutC()
    out.status, out.best_sample = 77, 78
    mask = np.full(40, 9, np.uint8)
    bad = s.copy()
    bad[2, 3] = 40
    neg = s.copy()
    neg[0, 0] = -1
    for bl, br, sm in ((c["bl"][:7], c["br"][:7], np.zeros((1, 8), np.int32)), (c["bl"], c["br"], bad), (c["bl"], c["br"], neg)):
        d = eng.two_view(bl, br, sm, out=out, inlier=mask, check=False)
        assert d["rc"] == -1  # LFVIO_ERR_ARG
        assert (out.status, out.best_sample) == (77, 78) and np.all(mask == 9)
    tin = abi.TwoViewInC()
    tin.num_matches, tin.num_samples = 40, 5
    assert eng.lib.lfvio_two_view(eng.ctx, C.byref(tin), mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out), None, None) == -1
    assert eng.lib.lfvio_two_view(eng.ctx, None, mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out), None, None) == -1
    assert (out.status, out.best_sample) == (77, 78)
    small = eng.two_view(c["bl"], c["br"], s)
    big_c, big_s = gen.make_case(53, 3000), gen.make_samples(54, 3000, 200)
    big = eng.two_view(big_c["bl"], big_c["br"], big_s, all_hypotheses=True)
    r = tv.two_view(big_c["bl"], big_c["br"], big_s)
    assert big["best_sample"] == r["best_sample"] and np.array_equal(big["mask"], r["mask"]) and np.array_equal(big["score_all"], r["score_all"])
    again = eng.two_view(c["bl"], c["br"], s)
    assert again["best_sample"] == small["best_sample"] and np.array_equal(again["E"], small["E"]) and np.array_equal(again["R_rel"], small["R_rel"])


@pytest.mark.gpu
def test_beside_an_optimization_in_flight(eng):
    """Test 6b: between lfvio_batch_optimize_begin and _finish, interleaved with lfvio_triangulate — the optimization's
    state and prior are the bits of the call without anything in between, and the two-view result is the bits of a call
    on an idle context."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    w = synth.make_window(0, 300)
    c, s = gen.make_case(61, 150, outliers=0.1), gen.make_samples(62, 150, 100)
    alone = eng.two_view(c["bl"], c["br"], s, all_hypotheses=True)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    def between(e):
        tin = abi.TriangulateIn(w)
        d0 = e.triangulate(tin, np.full(w.N, -1.0))
        tvr = e.two_view(c["bl"], c["br"], s, all_hypotheses=True)
        d1 = e.triangulate(tin, np.full(w.N, -1.0))
        assert np.array_equal(d0, d1)
        return tvr

    sol0, prior0, _ = split(Engine(0), None)
    sol1, prior1, tvr = split(Engine(0), between)
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    for k in ("E_all", "score_all", "E", "mask", "R_cand", "t_cand", "front", "R_rel"):
        assert np.array_equal(tvr[k], alone[k]), k
    assert (tvr["best_sample"], tvr["num_inliers"]) == (alone["best_sample"], alone["num_inliers"])
