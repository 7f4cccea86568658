"""Wall time of lfvio_solve against lfvio_solve_relo on the same 300-landmark window (one process, one device).

The relo solve carries K = 60 relocalization factors (synth.relo_message: a loop to an old keyframe 4 cm / 1.5 deg from
window frame 9).  Prints median and p95 over `--calls` calls of each, with the trust-region passes of the last call, and
one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd"))

from lfvio import synth  # noqa: E402
from lfvio.engine import Engine  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.percentile(t, 95))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--landmarks", type=int, default=300)
    ap.add_argument("--matches", type=int, default=60)
    a = ap.parse_args()
    eng = Engine(0)
    w = synth.make_window(0, a.landmarks)
    m = synth.relo_message(w, 9, a.matches, offset=((0.04, -0.02, 0.01), 1.5))
    K = len(m["landmark"])
    med_s, p95_s = timed(lambda: eng.solve(w), a.calls, a.warmup)
    passes_s = eng.last_passes()
    med_r, p95_r = timed(lambda: eng.solve_relo(w, 9, w.pose[9], m["landmark"], m["match_point"]), a.calls, a.warmup)
    passes_r = eng.last_passes()
    sol, _ = eng.solve_relo(w, 9, w.pose[9], m["landmark"], m["match_point"])
    print(f"lfvio_solve       N={w.N}: median {med_s:.3f} ms  p95 {p95_s:.3f} ms  passes {passes_s}")
    print(f"lfvio_solve_relo  N={w.N} K={K}: median {med_r:.3f} ms  p95 {p95_r:.3f} ms  passes {passes_r}  "
          f"iterations {sol.c.num_iterations}")
    print(json.dumps(dict(landmarks=w.N, matches=K, calls=a.calls, solve_ms_median=med_s, solve_ms_p95=p95_s, solve_passes=passes_s,
                          relo_ms_median=med_r, relo_ms_p95=p95_r, relo_passes=passes_r, relo_iterations=sol.c.num_iterations)))
    eng.close()


if __name__ == "__main__":
    main()
