"""The windows of tests/test_spec_candidates.py and the arithmetic on their traces (CPU only: no GPU, no library).

A pass of the trust-region loop of a small window prepares K candidates — the dogleg steps for radius, radius / 2, .. radius / 2^(K - 1)
— and the bookkeeping (csrc/tr_decide.h, decide_walk) takes them in that order: a rejected step halves the radius and the next candidate
is the step for that radius; the walk stops at the first accepted, invalid or terminating one.  Which candidate slot an accepted step
comes from is therefore decided by the run of rejections in front of it: after r rejections the step is candidate r mod K of its pass.
The windows below are chosen (scanned with oracle.binding.solve) for those runs; test_spec_candidates.py::test_oracle_runs holds that
the list still has them."""
from lfvio import abi, synth

# (seed, landmarks, max_num_iterations) of synth.make_window.  Sizes: one landmark, under a block (7, 33), one block and one past it
# (64, 65), several blocks (200) and SPEC_MAX_LM = 320 (the last block of cost_partE).  max_num_iterations 8 is the product's; with 16
# the synthetic windows reach the noise floor and reject, then accept.
# The oracle's steps behind each (A accepted, R rejected): the runs of rejections in front of an acceptance, and what the cap cut off.
CASES = (
    (1, 1, 8),      # AAARRRRR            the cap behind 5 rejections
    (3, 7, 8),      # AAARRRRA            a run of 4
    (14, 7, 8),     # AAARRRAA            3
    (2, 64, 8),     # AAAAAARR            the cap behind 2
    (13, 200, 8),   # AAAARRAA            2, past one block
    (9, 320, 8),    # AAARRRRA            4, five blocks
    (3, 7, 16),     # AAARRRRARRAAAAAA    4, 2
    (0, 7, 16),     # AAAAAAARRRRRARRA    5, 2
    (4, 1, 16),     # AAARRRRRRRRRAARA    9, 1
    (6, 33, 16),    # AAAAAAAARRRRRRAA    6
    (1, 64, 16),    # AAAAARRRARARRRRR    3, 1, the cap behind 5
    (17, 65, 16),   # AAAAAARRRRARRARA    4, 2, 1
    (8, 65, 16),    # AAAARRRRARAARARR    4, 1, 1, the cap behind 2
    (14, 120, 16),  # AAARRRAAAAAAAAAR    3, the cap behind 1
    (10, 300, 16),  # AAAAARRRRRARRAAR    5, 2, the cap behind 1
    (22, 320, 16),  # AAAAAAAAARRRAAAR    3, the cap behind 1
)
SPEC_MAX_LM = 320
RUN_LENGTHS = (1, 2, 3, 4, 5)  # 5: five or more


def case_id(case):
    return "seed%d-n%d-it%d" % case


def window(case):
    seed, n, max_iter = case
    return synth.make_window(seed, n, max_num_iterations=max_iter)


def steps(sol):
    """The iterations of a solution's trace as a string, entry 0 (the evaluation at the start) left out:
    'A' an accepted step, 'R' a rejected one, 'I' an invalid one."""
    c = sol.c
    return "".join("I" if not c.trace[k].step_is_valid else ("A" if c.trace[k].step_is_successful else "R")
                   for k in range(1, min(c.num_iterations, abi.MAX_TRACE)))


def runs(s):
    """steps() -> (the lengths of the runs of rejections that end in an accepted step, the rejections the string ends on).
    An invalid step ends a run without an acceptance: it is neither."""
    accepted, r = [], 0
    for ch in s:
        if ch == "R":
            r += 1
        else:
            if ch == "A" and r > 0:
                accepted.append(r)
            r = 0
    return accepted, r


def ends_on_cap(sol, max_iter):
    """The loop stopped because iteration max_iter was its last (NO_CONVERGENCE), not on a tolerance."""
    return sol.c.termination == abi.NO_CONVERGENCE and len(steps(sol)) == max_iter


def bucket(r):
    return min(r, RUN_LENGTHS[-1])


def run_histogram(sols):
    """{run length (the last of RUN_LENGTHS: that or longer): how many runs of rejections of that length end in an acceptance}"""
    h = {k: 0 for k in RUN_LENGTHS}
    for sol in sols:
        for r in runs(steps(sol))[0]:
            h[bucket(r)] += 1
    return h


def events(sol, max_iter):
    """The candidates the bookkeeping looked at, in order: steps(), and behind them 'T' where the loop ended on a candidate that met a
    tolerance — Minimize() returns before that iteration is recorded, but a pass had to prepare it.  (A loop that ends on the iteration
    cap ends with its last recorded step.)"""
    s = steps(sol)
    if ends_on_cap(sol, max_iter):
        return s
    assert sol.c.termination == abi.CONVERGENCE and len(s) < max_iter, (sol.c.termination, s)
    return s + "T"


def model_passes(ev, K):
    """Passes of the loop over the candidates `ev` (events()) with K candidates a pass: a pass ends at the first candidate that is not a
    rejection — accepted, invalid or terminating —, at the end of the loop, or after K candidates."""
    passes = i = 0
    while i < len(ev):
        passes += 1
        for z in range(K):
            i += 1
            if ev[i - 1] != "R" or i == len(ev):
                break
    return passes


def accepted_slots(ev, K):
    """The candidate slot z of every accepted step under K candidates a pass (model_passes' walk)."""
    out, i = [], 0
    while i < len(ev):
        for z in range(K):
            i += 1
            if ev[i - 1] == "A":
                out.append(z)
            if ev[i - 1] != "R" or i == len(ev):
                break
    return out


def largest_speculating_batch(source, n_landmarks, lm_block=64):
    """The largest batch of windows of n_landmarks landmarks whose passes still prepare several candidates, by the rule as it stands in
    loop_graphs (`source`: the text of csrc/lfvio_hip.hip): count * (landmark blocks + WINDOW_SIZE + 1) <= limit."""
    import re

    m = re.search(r"const bool speculate = \(size_t\)count \* \(g\.lm \+ LFVIO_WINDOW_SIZE \+ 1\) <= (\d+);", source)
    assert m, "loop_graphs: the rule that decides `speculate` is not where this test reads it"
    blocks = max(1, (n_landmarks + lm_block - 1) // lm_block)
    return int(m.group(1)) // (blocks + abi.WINDOW_SIZE + 1)
