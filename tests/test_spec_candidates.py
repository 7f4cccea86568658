"""Speculative trust-region candidates: the same bytes for every count and every history (tests/spec_cases.py holds the windows).

A pass of the loop of a small window prepares K dogleg steps at once — k_dogleg / k_step build candidate z for radius / 2^z into xE /
tabE / lamE / cost_partE, k_cost evaluates them all, decide_walk (csrc/tr_decide.h) takes them in Ceres' order and copy_accepted moves an
accepted extra candidate into the regular slot.  K is 3, or 4 behind a call whose steps were mostly rejected (loop_graphs), so the
answer of a product call must not depend on it: the radii are exact halvings either way, a pass that re-uses the linearization takes
the norms from the header, the cost kernels are the same for every candidate.  Held here:

  1  test_oracle_runs (CPU): the windows have what the candidate arrays can get wrong — runs of 1, 2, 3, 4 and more rejections in front
     of an accepted step (under K = 4: acceptance at z = 1, 2, 3 and a pass with every candidate rejected), also past one landmark block,
     and loops that meet the iteration cap in the middle of a pass;
  2  test_same_bytes_for_every_count: spec_count 2, 3, 4 give the bytes of spec_count 1 — state, inverse depths, summary, trace, prior —
     for both marginalization flags, in contexts that are re-used from window to window; test_switches_and_split_call: the same without
     captured graphs, without worker streams and through lfvio_batch_optimize_begin / _finish; test_device_runs: the DEVICE's own traces
     have the runs (near the noise floor it may accept where the oracle rejects);
  3  test_candidates_are_used: the pass counts "last_call" reports are the ones a model of the walk predicts from the count-1 trace,
     so a library that ignored the key would not pass 2 by doing nothing;
  4  test_history: one adaptive context, alternating between a window whose steps are mostly rejected and one whose are not: the
     target solved behind either — with 4 candidates, with 3, replaying both captured graph variants — gives the bytes of a fresh context;
  5  test_batches: three windows with different runs, and the largest batch that still speculates, at spec_count 1 and 4.

Every comparison is test_first_round.same: bytes, no tolerance."""
import os

import pytest

import spec_cases as sc
from lfvio.engine import Engine
from test_first_round import FLAGS, same

gpu = pytest.mark.gpu
COUNTS = (1, 2, 3, 4)
IDS = [sc.case_id(c) for c in sc.CASES]
VARIANT_CASE = (17, 65, 16)  # rejections in runs of 4, 2 and 1, two landmark blocks
# the history test: one landmark each, so that the three windows share the launch dimensions the captured graphs are kept under
HIST_REJECTED, HIST_ACCEPTED, HIST_TARGET = (19, 1, 16), (1, 1, 8), (4, 1, 16)
TRIO = ((3, 7, 16), (13, 200, 8), (22, 320, 16))
HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lf-vio_amd", "csrc", "lfvio_hip.hip")


@pytest.fixture(scope="module")
def wins():
    return {c: sc.window(c) for c in set(sc.CASES) | {HIST_REJECTED, HIST_ACCEPTED, HIST_TARGET}}


@pytest.fixture(scope="module")
def oracle_sols(oracle, wins):
    return {c: oracle.solve(wins[c]) for c in sc.CASES}


# ---- 1: the cases (CPU)
def test_case_list():
    sizes = {n for _, n, _ in sc.CASES}
    assert {1, 7, 33, 64, 65, sc.SPEC_MAX_LM} <= sizes and any(120 <= n <= 300 for n in sizes) and max(sizes) <= sc.SPEC_MAX_LM
    assert {it for _, _, it in sc.CASES} == {8, 16} and len(set(sc.CASES)) == len(sc.CASES)


def test_oracle_runs(oracle_sols):
    """Over the list the oracle meets every run length three times (the device, which may accept where the oracle rejects near the
    noise floor, has to meet each once: test_device_runs), each past one landmark block, and the cap after 1, 2 and >= 3 rejections."""
    assert all("I" not in sc.steps(s) for s in oracle_sols.values())
    h = sc.run_histogram(oracle_sols.values())
    assert all(h[k] >= 3 for k in sc.RUN_LENGTHS), h
    big = sc.run_histogram(s for c, s in oracle_sols.items() if c[1] > 64)
    assert all(big[k] >= 1 for k in sc.RUN_LENGTHS), big
    trailing = {min(sc.runs(sc.steps(s))[1], 3) for c, s in oracle_sols.items() if sc.ends_on_cap(s, c[2])}
    assert {1, 2, 3} <= trailing, trailing


def test_pass_model():
    """The arithmetic itself, on strings: 'AAARRRRA' is 8 passes one candidate at a time; with 3 the four rejections take two passes
    and the acceptance behind them is candidate 1 of the second, with 4 they fill one pass and the acceptance opens the next."""
    assert sc.runs("AAARRRRARAARR") == ([4, 1], 2) and sc.runs("RIRA") == ([1], 0)
    assert [sc.model_passes("AAARRRRA", k) for k in COUNTS] == [8, 6, 5, 5]
    assert sc.accepted_slots("AAARRRRA", 3) == [0, 0, 0, 1] and sc.accepted_slots("AAARRRRA", 4) == [0, 0, 0, 0]
    assert sc.accepted_slots("ARARRARRRA", 4) == [0, 1, 2, 3]
    assert [sc.model_passes("AARRT", k) for k in COUNTS] == [5, 4, 3, 3]  # (the candidate that met a tolerance rides in the rejections' pass)
    assert [sc.model_passes("RRRRRR", k) for k in COUNTS] == [6, 3, 2, 2]
    with open(HIP_SOURCE) as f:
        n = sc.largest_speculating_batch(f.read(), 64)
    assert n >= 3  # (test_batches runs a batch of that size and one larger)


# ---- the device
CAP_N = sc.SPEC_MAX_LM


def solve(eng, w, flag, cap_m, split=False):
    eng.batch_reserve(1, CAP_N, cap_m)
    eng.batch_upload(0, w)
    if split:
        sol = eng.optimize_begin(flag, w.N)
        return sol, eng.optimize_finish()
    eng.batch_optimize(1, flag)
    return eng.batch_download(0, w.N)


@pytest.fixture(scope="module")
def engines():
    """One context per candidate count, re-used by every case, flag and switch of this module."""
    es = {}
    for k in COUNTS:
        es[k] = Engine(0)
        es[k].set_spec_count(k)
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def solved(engines, wins):
    """(case, flag, count) -> (solution, prior) and -> "last_call", every case solved once per flag and count."""
    cap_m = max(wins[c].M for c in sc.CASES)
    out, calls = {}, {}
    for c in sc.CASES:
        for flag in FLAGS:
            for k in COUNTS:
                out[c, flag, k] = solve(engines[k], wins[c], flag, cap_m)
                calls[c, flag, k] = engines[k].last_call()
    return out, calls, cap_m


@gpu
@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_same_bytes_for_every_count(solved, case):
    out, calls, _ = solved
    for flag in FLAGS:
        for k in COUNTS[1:]:
            same(out[case, flag, k], out[case, flag, 1])
        assert bytes(out[case, flag, 1][0].c.trace) == bytes(out[case, FLAGS[0], 1][0].c.trace)  # (the loop does not know the flag)


@gpu
def test_workers_ran(engines, solved):
    """The contexts above start the marginalization of every accepted state on worker streams (spec_on): also of a state that was
    accepted as a speculative candidate."""
    for k in COUNTS:
        assert engines[k].marg_ahead()[0] > 0, k


@gpu
def test_device_runs(solved):
    """Coverage is a condition: what has to be the same bytes has to have happened.  In the device's count-1 traces: rejections in runs
    of 1, 2, 3 and >= 4 in front of an accepted step — under 4 candidates acceptance at z = 1, 2, 3 and a pass rejected whole."""
    out, calls, _ = solved
    sols = {c: out[c, FLAGS[0], 1][0] for c in sc.CASES}
    h = sc.run_histogram(sols.values())
    big = sc.run_histogram(s for c, s in sols.items() if c[1] > 64)
    slots = {k: sorted({z for c, s in sols.items() for z in sc.accepted_slots(sc.events(s, c[2]), k)}) for k in COUNTS}
    trailing = sorted({sc.runs(sc.steps(s))[1] for c, s in sols.items() if sc.ends_on_cap(s, c[2])})
    print("\ndevice traces:", {sc.case_id(c): sc.steps(s) for c, s in sols.items()})
    print("runs of rejections in front of an acceptance:", h, "past one block:", big, "accepted slots per count:", slots,
          "rejections in front of the cap:", trailing)
    assert h[1] >= 1 and h[2] >= 1 and h[3] >= 1 and h[4] + h[5] >= 1, h
    assert slots[4] == [0, 1, 2, 3] and slots[3] == [0, 1, 2] and slots[2] == [0, 1], slots


@gpu
def test_candidates_are_used(solved):
    """The windows whose trace has no invalid step: every count reports the iterations of count 1 and the passes the walk needs with
    that many candidates — which the model has to get right for count 1 first (one candidate a pass: a pass per candidate)."""
    out, calls, _ = solved
    table, covered = {}, 0
    for c in sc.CASES:
        for flag in FLAGS:
            sol = out[c, flag, 1][0]
            if "I" in sc.steps(sol):
                continue
            covered += 1
            ev = sc.events(sol, c[2])
            got = [calls[c, flag, k][0] for k in COUNTS]
            table[sc.case_id(c), flag] = (ev, got)
            assert calls[c, flag, 1][0] == sc.model_passes(ev, 1) == len(ev), (c, flag, ev, got)
            assert got == [sc.model_passes(ev, k) for k in COUNTS], (c, flag, ev, got)
            # (the header counts as Ceres does, from 1 at the first candidate: the entries of the trace, the evaluation at the start included —
            # also where the loop went on in continuation chunks behind the first graph, as it does with one candidate a pass)
            assert {calls[c, flag, k][1] for k in COUNTS} == {sol.c.num_iterations}, (c, flag, [calls[c, flag, k] for k in COUNTS])
            assert [calls[c, flag, k][3] for k in COUNTS] == list(COUNTS)
    print("\npasses per spec_count 1, 2, 3, 4:", table)
    print("sum over the windows:", [sum(g[k] for _, g in table.values()) for k in range(4)])
    assert covered >= len(sc.CASES)  # (at least half of the runs above; on the oracle no window has an invalid step)


@gpu
@pytest.mark.parametrize("variant", ["graph_off", "marg_ahead_off", "split_call"])
def test_switches_and_split_call(engines, solved, wins, variant):
    """One case without captured graphs, with the serial tail, and through lfvio_batch_optimize_begin / _finish (the graph variants that
    publish the state): under each, counts 2, 3, 4 give the bytes of count 1."""
    out, _, cap_m = solved
    key, off, on = {"graph_off": ("graph", 0, 1), "marg_ahead_off": ("marg_ahead", 0, 1), "split_call": (None, 0, 0)}[variant]
    w = wins[VARIANT_CASE]
    for flag in FLAGS:
        got = {}
        for k in COUNTS:
            if key:
                engines[k].configure(key, off)
            try:
                got[k] = solve(engines[k], w, flag, cap_m, split=variant == "split_call")
            finally:
                if key:
                    engines[k].configure(key, on)
        for k in COUNTS[1:]:
            same(got[k], got[1])
        if variant != "graph_off":  # (worker streams or not, whole call or split: the same bytes by test_marg_ahead.py and test_early_solution.py)
            same(got[1], out[VARIANT_CASE, flag, 1])


# ---- 4: history
@gpu
def test_history(wins):
    """Adaptive count on one context: H (steps mostly rejected) makes the next call prepare 4 candidates, A (8 iterations in 5 passes) 3.
    The target T behind either is the bytes of a fresh context; three alternations, so that both variants of the captured graphs are
    replayed, not only captured.  "last_call" [3] behind T is the count T ran with: the two values are what the test stands on."""
    H, A, T = wins[HIST_REJECTED], wins[HIST_ACCEPTED], wins[HIST_TARGET]
    cap_m = max(w.M for w in (H, A, T))
    for flag in FLAGS:
        ref = Engine(0)
        want = solve(ref, T, flag, cap_m)
        assert ref.last_call()[3] == 3  # (a fresh context prepares 3)
        ref.close()
        assert sc.runs(sc.steps(want[0]))[0], "the target has no rejected-then-accepted run"
        eng = Engine(0)
        seen = []
        for rep in range(3):
            for first, count in ((H, 4), (A, 3)):
                solve(eng, first, flag, cap_m)
                passes, iters = eng.last_call()[:2]
                assert (iters >= 2 * passes) == (count == 4), (rep, count, passes, iters)
                same(solve(eng, T, flag, cap_m), want)
                seen.append(eng.last_call()[3])
                assert seen[-1] == count, seen
        eng.close()


# ---- 5: batches
@pytest.fixture(scope="module")
def batch_engines():
    es = {}
    for k in (1, 4):
        es[k] = Engine(0)
        es[k].set_spec_count(k)
    yield es
    for e in es.values():
        e.close()


def run_batch(eng, ws, flag, slots):
    eng.batch_reserve(slots, max(w.N for w in ws), max(w.M for w in ws))
    for s, w in enumerate(ws):
        eng.batch_upload(s, w)
    eng.batch_optimize(len(ws), flag)
    return [eng.batch_download(s, w.N) for s, w in enumerate(ws)], eng.last_call()[0]


@gpu
def test_batches(batch_engines, solved, wins):
    """Three windows with different runs (7, 200 and 320 landmarks), and the largest batch of one-block windows that still speculates by
    the rule in loop_graphs — read from there: each slot the same bytes at spec_count 1 and 4, and the bytes of its window solved alone.
    The pass counts say that the batches did speculate, and that one window more would not."""
    out, _, _ = solved
    with open(HIP_SOURCE) as f:
        largest = sc.largest_speculating_batch(f.read(), 64)
    small = [c for c in sc.CASES if c[1] <= 64]
    assert len(small) >= 3 and largest + 1 <= 64
    full = [small[s % len(small)] for s in range(largest + 1)]
    for cases in (TRIO, full[:largest]):
        for flag in FLAGS:
            got = {k: run_batch(batch_engines[k], [wins[c] for c in cases], flag, largest + 1) for k in (1, 4)}
            for s, c in enumerate(cases):
                same(got[4][0][s], got[1][0][s])
                same(got[1][0][s], out[c, flag, 1])
            evs = [sc.events(out[c, flag, 1][0], c[2]) for c in cases]
            if all("I" not in ev for ev in evs):
                want = {k: max(sc.model_passes(ev, k) for ev in evs) for k in (1, 4)}
                print("\nbatch of", len(cases), "passes at spec_count 1, 4:", got[1][1], got[4][1])
                assert (got[1][1], got[4][1]) == (want[1], want[4]) and want[4] < want[1], (len(cases), got[1][1], got[4][1], want)
    # one window more: the rule says no candidates beyond the first, whatever the key
    flag = FLAGS[0]
    sols, passes = run_batch(batch_engines[4], [wins[c] for c in full], flag, largest + 1)
    for s, c in enumerate(full):
        same(sols[s], out[c, flag, 1])
    evs = [sc.events(out[c, flag, 1][0], c[2]) for c in full]
    if all("I" not in ev for ev in evs):
        assert passes == max(len(ev) for ev in evs), (passes, [len(ev) for ev in evs])
