"""The step half of one trust-region pass — landmark back-substitution, ComputeTraditionalDoglegStep, Plus(x, delta), the candidate's cost at
every factor, the model cost change, Ceres' accept / reject / terminate bookkeeping — against a 50-digit reference (tests/step_hp.py).

Every other test sees these kernels through the end of a whole optimization() (states 1e-6, costs 1e-7), where a wrong d1 / d2 pair, an
observation missing from a cost loop or a missing factor 2 in the model only change which step is accepted, and the next passes absorb it.
Here ONE pass is run (lfvio_debug_step_io: the launches of the loop's own launch_step_half) and what each stage WROTE is held to a
50-digit statement of Ceres' and the reference's formulas evaluated on what that stage READ; the bookkeeping is restated in plain double on
the device's own sums (integers, radius and mu equal; the other doubles within bounds counted from the roundings of each chain,
step_hp.rounding_bounds), its discrete outcome must be that of a complete 50-digit pass, and an accepted speculative candidate must be in
x / lam / tab [cur] byte for byte.

Bars: 16 x the worst of two double-precision comparators (tests/np_ref.py with a LAPACK solve, the oracle/ build) on the same case list,
per metric and class (group, mu), the metrics that involve neither y nor the conditioning pooled (step_hp.POOLED) — measured and asserted
in the CPU tests below (step_hp.COMPARATOR_WORST); nothing is taken from the device.

Routes (lfvio_debug_configure) and shapes — the smallest at which each kernel can still go wrong, all windows from lfvio.synth, 11 frames:
  step     one window, defaults, spec 1 and 4: k_step at N = 0, 1, 7, 64, 65, 320; the variants at spec 2
  backsub  one window of 321 landmarks: k_backsub + k_dogleg<false> + k_cost<4> + k_decide;  backsub_wt: "linw" 2, k_backsub_wt in front
  stepw    a resident batch of 2, "linw" 2 (at 1 a batch of two stays on the role-by-role sweep): k_stepw at N = 64, 257, 320 and the variants, slot 1 checked
  batch    "linw" 0, the smallest batch with count x (blocks + 11) > 2048 — 171 windows of N = 7, first and last slot checked; 158 with the
           variants in its first slots (ocam_rs has two blocks), those checked: k_dogleg<true, false> + k_cost<1, false> + k_cost_imu + k_decide
Variants (prior, no_td, no_ex, no_td_no_ex, ocam_rs, skip_imu0: the constructors of tests/solve_cases.py) run on the routes a window of
their size can take: step, stepw, batch — a window of 64 or 120 landmarks never takes the routes of 321.

Measured, worst of the class, comparators / bar / device (MI355X, all five routes), in eps of the unit step_hp.py gives the metric:

  class          d2               gn_l             grad_gn_total    delta            cand_p           cand_lam         mcc              mlin             mquad            
  regular 1e-08  1.65/26.4/2.69   2.57/41.1/2.22   0.597/9.55/0.724 2.68/42.9/2.85   2.86/45.8/2.57   2.18/34.9/1.93   2.77/44.3/2.04   2.28/36.5/1.76   1.38/22.1/0.78   
  regular 0.01   1.92/30.7/3.28   3.28/52.5/2.89   0.787/12.6/0.787 2.82/45.1/3.2    2.52/40.3/2.57   1.78/28.5/1.99   2.57/41.1/3.06   2.28/36.5/1.66   1.14/18.2/0.78   
  weak 1e-08     1.38/22.1/1.41   2.02/32.3/1.22   1.11/17.8/1.41   3.08/49.3/2.64   2.5/40/2         1.48/23.7/1.68   1.81/29/1.03     1.64/26.2/2.12   2.3/36.8/2.09    
  weak 0.01      0.859/13.7/1.49  2.73/43.7/1.74   1.89/30.2/1.1    2.53/40.5/2.17   2.07/33.1/2.13   1.36/21.8/1.25   1.81/29/1.03     1.38/22.1/1.23   2.3/36.8/1.77    
  prior 1e-08    0.937/15/1.56    1.52/24.3/1.5    0.888/14.2/0.379 2.32/37.1/2.65   1.55/24.8/1.6    2.02/32.3/1.72   1.08/17.3/0.442  1.32/21.1/1.03   1.87/29.9/1.54   
  prior 0.01     1.38/22.1/0.922  4.17/66.7/1.69   1.15/18.4/1.38   2.66/42.6/2.65   0.99/15.8/0.984  1.7/27.2/1.86    1.18/18.9/1.25   1.69/27/0.858    0.859/13.7/1.49  
  solved 1e-08   1.18/18.9/1.02   1.28/20.5/1.02   0.644/10.3/0.544 2.2/35.2/2.32    0.937/15/0.922   0.975/15.6/0.989 2.45/39.2/1.14   1.17/18.7/0.971  1.08/17.3/2.04   

  pooled         d1 3.58/57.3/4.5   gn_sq_total 0.858/13.7/0.809   cg 1.25/20/1.54   cn 1.48/23.7/1.44   sn 1.95/31.2/1.95   cand_q 4.78/76.5/4.1
                 step_sq_pose 1.9/30.4/0.732   xn2_pose 3.97/63.5/2.49   dn 0.705/11.3/0.61   xn 1.86/29.8/2.07   gmax 0/0/0
                 vis_block 1.99/31.8/1.31   vis_total 1.03/16.5/1.28   imu_cost 0.745/11.9/0.678   prior_cost 0.00708/0.113/0.00783

The device sits at the comparators' own level in every metric of every route (0.4 x .. 1.9 x their worst): the per-pair table and the
rsqrt of the cost loops, the transposed rows of the inline back-substitution and the wave-level sums are as close to the 50-digit values as
numpy on the same inputs.  All 178 device passes reach the outcome of the 50-digit pass, the bookkeeping's doubles lie within the counted
roundings and its integers, radius and mu are equal.  prior_cost rests on ONE sample per run (the oracle exposes no prior evaluation, both
comparators take tests/np_ref.py's), gmax on the exact |g| of a speed / bias entry in every run (bar 0: the device must give that double).

Radii replaced after the CPU preconditions, none left out: case 1 runs at 2.5 |gn| — at 2 |gn| candidate 1 sits exactly on |gn| = r, at
3 |gn| the accepted Gauss-Newton step sits on radius = 3 |step|, the tie between a radius kept and a radius grown.
"""
import time

import numpy as np
import pytest

from lfvio import abi, synth
from lfvio.engine import Engine

import lin_cases as lc
import lin_hp as lh
import np_ref
import solve_cases as sc
import step_hp as sp

MU_A, MU_B = 1e-8, 1e-2
SIZES = ("imu_only", "n1", "n7", "n64", "n65", "n320")
VARIANTS = ("prior", "no_td", "no_ex", "no_td_no_ex", "ocam_rs", "skip_imu0")


def _solved(oracle):
    """n64 at the state three optimization() calls of the oracle leave: the gradient is at rounding level of its terms."""
    w = sc.window(oracle, "n64")
    for _ in range(3):
        w = abi.apply_solution(w, oracle.optimize(w, abi.MARGIN_OLD)[0])
    return w


EXTRA = {"n320": lambda o: lc.short_tracks(9, 320), "n321": lambda o: lc.short_tracks(10, 321), "n257": lambda o: lc.short_tracks(14, 257),
         "solved": _solved}
# the class of a case, known before anything is computed: (group, mu) — solve_cases.GROUP's groups, and "solved": at a solution the
# gradient is what is left of terms 1e6 times its size, and so is everything the step half forms from it
GROUP = dict(sc.GROUP, solved="solved")
_win = {}


def window(oracle, name):
    if name not in _win:
        _win[name] = EXTRA[name](oracle) if name in EXTRA else sc.window(oracle, name)
    return _win[name]


def case_class(name, mu):
    return (GROUP.get(name, "regular"), mu)


# A run: (window, mu, kind, K).  kind 1 / 2 / 3: the radius that puts candidate 0 into that dogleg case, from the np_ref comparator's norms at
# that mu — 2.5 |gn|, 0.5 alpha |g|, sqrt(alpha |g| |gn|); a float: that radius.  K: candidates (the device runs K and every smaller count asked for).
CASES3 = (1, 2, 3)
RUNS = ([(n, mu, k, 4) for n in SIZES for mu in (MU_A, MU_B) for k in CASES3]
        + [(n, mu, k, 2) for n in VARIANTS for mu in (MU_A, MU_B) for k in CASES3]
        + [(n, mu, k, 1) for n in ("n257",) for mu in (MU_A, MU_B) for k in CASES3]
        + [("n321", MU_A, 3, 1)]
        # the outcomes the dogleg cases do not give: a reject, a reject and then an accept, an accept that halves the radius, the function
        # tolerance (all at the solution), the parameter tolerance (a radius of 1e-12)
        + [("solved", MU_A, 1e4, 1), ("solved", MU_A, 0.6, 2), ("solved", MU_A, 0.6, 4), ("solved", MU_A, 0.2, 1), ("solved", MU_A, 1e-4, 1),
           ("n64", MU_A, 1e-12, 1)])


def _rid(v):
    """[route-]window-mu-case-K"""
    *head, kind, K = v
    return "-".join([f"{x:g}" if isinstance(x, float) else str(x) for x in head] + [f"case{kind}" if isinstance(kind, int) else f"r{kind:g}", f"K{K}"])


_norms, _stm, _ref, _cpu = {}, {}, {}, {}


def radius_of(oracle, name, mu, kind):
    if isinstance(kind, float):
        return kind
    if (name, mu) not in _norms:
        h = sp.comparator_pass(window(oracle, name), mu, 1e4, 1)["head"]
        _norms[(name, mu)] = (float(np.sqrt(h["gn_sq_total"])), float(h["alpha"] * np.sqrt(h["grad_sq_total"])))
    gn, cauchy = _norms[(name, mu)]
    # (case 1 at 2.5 |gn|, not 2 |gn|: candidate 1 of 2 |gn| sits exactly on |gn| = r, which the condition on the dogleg tests rules out —
    # and at 3 |gn| the accepted Gauss-Newton step would sit on radius = 3 |step|, the tie between a radius kept and a radius grown)
    return {1: 2.5 * gn, 2: 0.5 * cauchy, 3: float(np.sqrt(cauchy * gn))}[kind]


def statement(oracle, name):
    if name not in _stm:
        _stm[name] = lh.Statement(window(oracle, name), keep_mp=False)
    return _stm[name]


def reference(oracle, name, mu, radius, K):
    """The complete 50-digit pass of the run: computed once per session."""
    key = (name, mu, radius, K)
    if key not in _ref:
        _ref[key] = sp.reference_pass(window(oracle, name), statement(oracle, name), mu, radius, K)
    return _ref[key]


def cpu_run(oracle, run):
    """Both comparators through every stage, and the reference pass: computed once per session."""
    if run not in _cpu:
        name, mu, kind, K = run
        w, radius = window(oracle, name), radius_of(oracle, name, mu, kind)
        perm = lc.device_order(w)
        out = dict(w=w, radius=radius, perm=perm, ios={}, reps={})
        for tag, orc in (("np_ref", None), ("oracle", oracle)):
            io = sp.comparator_pass(w, mu, radius, K, orc)
            out["ios"][tag], out["reps"][tag] = io, sp.full_report(io, w, perm, io["states"], io["H"])
        out["ref"] = reference(oracle, name, mu, radius, K)
        _cpu[run] = out
    return _cpu[run]


def _line(tag, rep):
    return f"{tag}: cases {rep['cases']} " + " ".join(f"{k}={rep[k]:.3g}" for k in sp.ALL_METRICS)


def same_outcome(got, ref):
    return all(got[k] == ref[k] for k in ("kind", "acc_z", "entries", "done", "termination", "cur"))


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=[_rid(r) for r in RUNS])
def test_preconditions_and_comparators_inside_every_bar(oracle, run):
    """Every precondition of the run, on the CPU: both dogleg tests at least 1e-6 (relative) away from equality for every candidate, in
    the comparators and in the 50-digit pass; candidate 0 in the case asked for; relative_decrease at least 1e-3 (relative) away from
    1e-3, 0.25 and 0.75 and both tolerance tests from equality in the 50-digit pass; the comparators' cases and outcome are the
    reference's.  Then the comparators through every metric: this is where the bars come from (the printed figures are what
    step_hp.COMPARATOR_WORST holds)."""
    name, mu, kind, K = run
    R = cpu_run(oracle, run)
    ref = R["ref"]
    assert ref["margins"] >= 1e-3, ref
    for case, mg in ref["dogleg"]:
        assert min(abs(mg[0]), abs(mg[1])) >= 1e-6, ref["dogleg"]
    if not isinstance(kind, float):
        assert ref["dogleg"][0][0] == kind, (kind, ref["dogleg"])
    for tag, rep in R["reps"].items():
        print(_line(f"{_rid(run)} {tag}", rep))
        io = R["ios"][tag]
        assert rep["cases"] == rep["dev_cases"] and all(min(abs(m[0]), abs(m[1])) >= 1e-6 for m in rep["margins"]), (tag, rep["cases"], rep["margins"])
        assert rep["cases"][:len(ref["dogleg"])] == [c for c, _ in ref["dogleg"]], (tag, rep["cases"], ref["dogleg"])
        assert rep["exact"] and rep["skipped_zero"], tag
        assert same_outcome(sp.outcome_of(io["after"], io["trace"], io["acc_z"], R["radius"]), ref), (tag, ref)
        assert sp.bookkeeping_check(io)[0] == [], tag
    for tag, rep in R["reps"].items():
        assert sp.failed_checks(rep, sp.ALL_METRICS, case_class(name, mu)) == [], tag


def comparator_worst(oracle):
    worst = {}
    for run in RUNS:
        cls = case_class(run[0], run[1])
        for rep in cpu_run(oracle, run)["reps"].values():
            for k in sp.ALL_METRICS:
                for c in (cls, "all"):
                    worst.setdefault(c, {})
                    worst[c][k] = max(worst[c].get(k, 0.0), rep[k])
    return {c: {k: float(f"{v:.3g}") for k, v in d.items() if (c == "all") == (k in sp.POOLED)} for c, d in worst.items()}


def test_comparator_table_reproduces(oracle):
    """step_hp.COMPARATOR_WORST is the worst figure of the two comparators over RUNS, to the three digits it is written with."""
    worst = comparator_worst(oracle)
    print("COMPARATOR_WORST = " + repr(worst))
    assert set(worst) == set(sp.COMPARATOR_WORST)
    for c, d in worst.items():
        for k, v in d.items():
            assert abs(v - sp.COMPARATOR_WORST[c][k]) <= 5e-3 * max(v, sp.COMPARATOR_WORST[c][k]), (c, k, v, sp.COMPARATOR_WORST[c][k])


def test_case_list_covers_what_it_must(oracle):
    """A track of 2 and one of 11 observations, the widest prior synth.make_window_with_prior yields (76 columns: ten poses, one speed / bias,
    ex, td — the most MARGIN_OLD keeps), a skipped IMU factor; every outcome: accepted with the radius grown, accepted with it kept or halved,
    rejected, function-tolerance and parameter-tolerance convergence, and — with two candidates or more — candidate 0 rejected and
    candidate 1 accepted."""
    lens = set()
    for n in set(r[0] for r in RUNS):
        lens |= set(np.diff(window(oracle, n).obs_offset).tolist())
    assert 2 in lens and 11 in lens
    assert window(oracle, "prior").prior.n == 76 == max(synth.make_window_with_prior(s, 64, oracle.optimize)[0].prior.n for s in (1, 2))
    assert window(oracle, "skip_imu0").imu[0].sum_dt > 10.0
    kinds = {}
    for run in RUNS:
        name, mu, kind, K = run
        ref = reference(oracle, name, mu, radius_of(oracle, name, mu, kind), K)
        kinds.setdefault(ref["kind"], []).append(run)
        if ref["kind"] == "converged":
            kinds.setdefault("parameter_tolerance" if kind == 1e-12 else "function_tolerance", []).append(run)
        if K >= 2 and ref["acc_z"] == 1 and ref["entries"] == 2:
            kinds.setdefault("rejected_then_accepted", []).append(run)
    print({k: len(v) for k, v in kinds.items()})
    for k in ("accepted_grown", "accepted_kept_or_halved", "rejected", "function_tolerance", "parameter_tolerance", "rejected_then_accepted"):
        assert kinds.get(k), k
    # the tiny radius ends on the parameter tolerance, the solution on the function tolerance: the first test that fires in the 50-digit pass
    r = reference(oracle, "n64", MU_A, 1e-12, 1)
    assert r["kind"] == "converged" and r["entries"] == 0


def test_the_largest_reference_takes_seconds(oracle):
    w = window(oracle, "n321")
    t0 = time.time()
    stm = lh.Statement(w, keep_mp=False)
    sp.reference_pass(w, stm, MU_A, radius_of(oracle, "n321", MU_A, 3), 1)
    assert time.time() - t0 < 60.0


# ---- corrupted outputs: each stage's check fails when it should
def _copy(io):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in io.items()}
    out["head"], out["after"] = dict(io["head"]), dict(io["after"])
    out["trace"] = [dict(t) for t in io["trace"]]
    return out


def _failed(R, io, cls, states=None):
    rep = sp.full_report(io, R["w"], R["perm"], states or io["states"], io["H"])
    return [b[0] for b in sp.failed_checks(rep, sp.ALL_METRICS, cls)]


def test_corrupted_outputs_fail(oracle):
    run = ("n64", MU_A, 3, 4)
    R = cpu_run(oracle, run)
    cls = case_class("n64", MU_A)
    good = R["ios"]["np_ref"]
    assert _failed(R, good, cls) == []
    # a. d1 and d2 swapped
    io = _copy(good)
    io["d1"], io["d2"] = good["d2"].copy(), good["d1"].copy()
    bad = _failed(R, io, cls)
    print("d1 / d2 swapped:", bad)
    assert "d1" in bad and "d2" in bad and "mquad" in bad
    # a. gn_l of one landmark from its neighbour's W row
    io = _copy(good)
    l = 5
    io["gn_l"][l] = -good["diag_l"][l] * (good["scale_l"][l] * good["b"][l] + good["scale_l"][l] * (good["W"][l + 1] @ good["uc_gn"][:sp.KC])) * good["einv_l"][l]
    bad = _failed(R, io, cls)
    print("gn_l from the neighbour's row:", bad)
    assert "gn_l" in bad
    # b. a relative change of 1e-12 in cg
    io = _copy(good)
    io["coef"][0][0] *= 1.0 + 1e-12
    bad = _failed(R, io, cls)
    print("cg off by 1e-12:", bad)
    assert "cg" in bad
    # c. the quaternion not normalized
    io = _copy(good)
    st = dict(x=good["states"]["x"], cand=[{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()} for c in good["states"]["cand"]])
    x, d = st["x"]["pose"][3], good["step_p"][18:24]
    q = np_ref.qmul(np_ref.pose_q(x), np_ref.deltaQ(d[3:6]))
    st["cand"][0]["pose"][3, 3:] = [q[1], q[2], q[3], q[0]]
    bad = _failed(R, io, cls, st)
    print("quaternion not normalized:", bad, "defect", abs(np.linalg.norm(q) - 1.0))
    assert "cand_q" in bad
    # d. one observation missing from one track's cost
    io = _copy(good)
    w = R["w"]
    lcal = int(R["perm"][7])
    cand = good["states"]["cand"][0]
    o0, fi = int(w.obs_offset[lcal]), int(w.start_frame[lcal])
    o = int(w.obs_offset[lcal + 1]) - 1
    r = np_ref.visual(bool(w.estimate_td), w.tr, w.row, w.sqrt_info, w.obs_point[o0], w.obs_point[o], w.obs_velocity[o0], w.obs_velocity[o], w.obs_cur_td[o0],
                      w.obs_cur_td[o], w.obs_uv_y[o0], w.obs_uv_y[o], cand["pose"][fi], cand["pose"][fi + o - o0], cand["ex"], good["cand_lam"][0][7], cand["td"])[0]
    io["block_sums"][0, 0, 0] -= 0.5 * np.log(1 + r @ r)
    bad = _failed(R, io, cls)
    print("a track's last observation dropped:", bad, "its cost", 0.5 * np.log(1 + r @ r), "of", good["block_sums"][0, 0, 0])
    assert "vis_block" in bad and "vis_total" in bad
    # e. mquad without its factor 2
    io = _copy(good)
    dl = (good["coef"][0][0] * good["grad_l"] + good["coef"][0][1] * good["gn_l"]) / good["diag_l"] * good["scale_l"]
    wd = good["coef"][0][0] * good["d1"] + good["coef"][0][1] * good["d2"]
    io["block_sums"][0, 0, 2] = (dl * wd + good["a"] * dl * dl).sum()
    bad = _failed(R, io, cls)
    print("mquad without its factor 2:", bad)
    assert "mquad" in bad and "mcc" in bad
    # c. the inactive mask forgotten (td constant)
    run2 = ("no_td", MU_A, 3, 2)
    R2 = cpu_run(oracle, run2)
    g2 = R2["ios"]["np_ref"]
    io = _copy(g2)
    c0 = g2["coef"][0]
    io["step_p"][sp.OFF_TD] = (c0[0] * g2["grad_p"][sp.OFF_TD] + c0[1] * g2["gn_p"][sp.OFF_TD]) / g2["diag_p"][sp.OFF_TD] * g2["scale_p"][sp.OFF_TD] + 1e-9
    bad = _failed(R2, io, case_class("no_td", MU_A))
    print("inactive mask forgotten:", bad)
    assert "delta" in bad
    # f. a rejected step that leaves the radius unhalved
    run3 = ("solved", MU_A, 1e4, 1)
    R3 = cpu_run(oracle, run3)
    g3 = R3["ios"]["np_ref"]
    assert sp.bookkeeping_check(g3)[0] == []
    io = _copy(g3)
    io["after"]["radius"] = g3["head"]["radius"]
    io["trace"][0]["trust_region_radius"] = g3["head"]["radius"]
    bad = sp.bookkeeping_check(io)[0]
    print("rejected, radius unhalved:", bad)
    assert [b for b in bad if b[0] == "radius"]


# ------------------------------------------------------------------------------------------------------------------------
# GPU: one pass per run and route on the device, through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------
STEP, BACKSUB, BACKSUB_WT, STEPW, BATCH = "step", "backsub", "backsub_wt", "stepw", "batch"
# the smallest batch with count x (blocks + 11) > 2048: 171 windows of 7 landmarks (one block); with the variants in it (ocam_rs: two blocks) 158
BATCH_COUNT, BATCH_COUNT_VARIANTS = 171, 158
BATCH_SLOTS = {"n7": 0, "n7_last": BATCH_COUNT - 1, **{v: i for i, v in enumerate(VARIANTS)}}
DEVICE_RUNS = ([(STEP, n, mu, k, K) for (n, mu, k, K4) in RUNS if n in SIZES and K4 == 4 for K in (1, 4)]
               + [(STEP, n, mu, k, K) for (n, mu, k, K) in RUNS if n in VARIANTS or n in ("solved",) or k == 1e-12]
               + [(BACKSUB, "n321", MU_A, 3, 1), (BACKSUB_WT, "n321", MU_A, 3, 1)]
               + [(STEPW, n, mu, k, 1) for n in ("n64", "n257", "n320") + VARIANTS for mu in (MU_A, MU_B) for k in CASES3]
               + [(BATCH, n, MU_A, 3, 1) for n in BATCH_SLOTS])
_dev = dict(key=None)


@pytest.fixture(scope="module")
def dev(eng):
    yield eng
    eng.set_linw(1)


def _upload(dev, oracle, key, linw, windows):
    if _dev["key"] != key:
        dev.set_linw(linw)
        dev.batch_reserve(len(windows), max(max(w.N for w in windows), 1), max(max(w.M for w in windows), 1))
        for s, w in enumerate(windows):
            dev.batch_upload(s, w)
        _dev["key"] = key


def device_pass(dev, oracle, route, name, mu, radius, K):
    """The pass of the run on its route: (io, window)."""
    wname = "n7" if name == "n7_last" else name
    w = window(oracle, wname)
    if route in (STEP, BACKSUB, BACKSUB_WT):
        _upload(dev, oracle, (route, name), 2 if route == BACKSUB_WT else 1, [w])
        io = dev.step_io(1, 0, w.N, mu, radius, K, tabs=True)
        assert io["linw"] == (2 if route == BACKSUB_WT else 0) and io["stepw"] == 0 and io["head_valid"] == 1
    elif route == STEPW:
        # ("linw" 2: at 1 a batch of two stays on the role-by-role sweep — the strip sweep is the default only for a batch large enough to split)
        _upload(dev, oracle, (route, name), 2, [window(oracle, "n7"), w])
        io = dev.step_io(2, 1, w.N, mu, radius, 1, tabs=True)
        assert io["linw"] == 1 and io["stepw"] == 1 and io["head_valid"] == 0
    else:
        var = name in VARIANTS
        count = BATCH_COUNT_VARIANTS if var else BATCH_COUNT
        ws = [window(oracle, "n7")] * count
        for v in VARIANTS if var else ():
            ws[BATCH_SLOTS[v]] = window(oracle, v)
        nb = max((x.N + 63) // 64 for x in ws) + 11
        assert count * nb > 2048 and (count - 1) * nb <= 2048
        _upload(dev, oracle, (route, var), 0, ws)
        io = dev.step_io(count, BATCH_SLOTS[name], w.N, mu, radius, 1, tabs=True)
        assert io["linw"] == 0 and io["stepw"] == 0 and io["head_valid"] == 1
    return io, w


def device_states(io):
    return dict(x=Engine.state_dict(io["x"]), cand=[Engine.state_dict(io["cand_x"][z]) for z in range(io["spec"])])


@pytest.mark.gpu
@pytest.mark.parametrize("drun", DEVICE_RUNS, ids=[_rid(r) for r in DEVICE_RUNS])
def test_device_pass(dev, oracle, drun):
    route, name, mu, kind, K = drun
    wname = "n7" if name == "n7_last" else name
    radius = radius_of(oracle, wname, mu, kind)
    io, w = device_pass(dev, oracle, route, name, mu, radius, K)
    cls = case_class(wname, mu)
    h = io["head"]
    assert io["chol_fail"] == 0 and h["mu"] == mu and h["radius"] == radius and h["done"] == 0 and io["spec"] == K, (io["chol_fail"], h, io["spec"])
    assert (io["est_ex"], io["est_td"]) == (w.estimate_extrinsic, w.estimate_td)
    perm = lc.device_order(w)
    assert np.array_equal(io["lam"], w.inv_depth[perm]) and np.array_equal(io["x"][:77].reshape(11, 7), w.pose)
    states = device_states(io)
    rep = sp.full_report(io, w, perm, states)
    print(_line(f"{_rid(drun)} device", rep))
    # b. the discrete case of every candidate, given that both tests are 1e-6 away from equality on the device's own totals
    assert all(min(abs(m[0]), abs(m[1])) >= 1e-6 for m in rep["margins"]) and rep["cases"] == rep["dev_cases"], (rep["cases"], rep["dev_cases"], rep["margins"])
    if not isinstance(kind, float):
        assert rep["cases"][0] == kind
    # c. exact properties: constant blocks copied, zero step in their columns
    act = sp.active_pose(io["est_ex"], io["est_td"])
    assert rep["exact"] and np.all(io["step_p"][~act] == 0.0)
    # d. a skipped factor and a missing prior cost exactly nothing
    assert rep["skipped_zero"]
    # f. the bookkeeping on the device's own sums, and the outcome of the complete 50-digit pass
    bad, want, trace, acc_z = sp.bookkeeping_check(io)
    ref = reference(oracle, wname, mu, radius, K)
    dev_acc = len(io["trace"]) - 1 if io["trace"] and io["trace"][-1]["step_is_successful"] else -1
    got = sp.outcome_of(io["after"], io["trace"], dev_acc, radius)
    print(f"{_rid(drun)} outcome {got} reference margins {ref['margins']:.3g}")
    assert bad == [] and dev_acc == acc_z
    assert same_outcome(got, ref), (got, ref)
    # g. the accepted candidate is the state: byte for byte (a speculative one was copied over candidate 0's slot)
    if acc_z >= 0:
        assert io["x_after"].tobytes() == io["cand_x"][acc_z].tobytes() and io["lam_after"].tobytes() == io["cand_lam"][acc_z].tobytes()
        assert io["tab_after"].tobytes() == io["cand_tab"][acc_z].tobytes()
    else:
        assert io["x_after"].tobytes() == io["x"].tobytes() and io["lam_after"].tobytes() == io["lam"].tobytes()
    assert sp.failed_checks(rep, sp.ALL_METRICS, cls) == []


DETERMINISM = [(STEP, "n65", 4), (BACKSUB, "n321", 1), (BACKSUB_WT, "n321", 1), (STEPW, "n257", 1), (BATCH, "n7_last", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("route,name,K", DETERMINISM, ids=[d[0] for d in DETERMINISM])
def test_device_two_runs_give_the_same_bytes(dev, oracle, route, name, K):
    radius = radius_of(oracle, "n7" if name == "n7_last" else name, MU_A, 3)
    a, _ = device_pass(dev, oracle, route, name, MU_A, radius, K)
    b, _ = device_pass(dev, oracle, route, name, MU_A, radius, K)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
    for k in ("head", "after"):
        for f, v in a[k].items():
            assert (v.tobytes() == b[k][f].tobytes()) if isinstance(v, np.ndarray) else (v == b[k][f] or (v != v and b[k][f] != b[k][f])), (k, f)
    assert repr(a["trace"]) == repr(b["trace"])
