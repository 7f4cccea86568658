"""lfvio_sfm_ba at F = 11, P in {60, 300, 1000} (ragged tracks, 1 px noise, the 1.5 degree / 3 % / 5 % start of the fixtures), default
options: median / p95 of the whole call (host buffers in / out) over 20 calls after 3 warm-up calls, beside the numpy restatement
(tests/sfm_ba_ref.py — numpy, not a tuned C++ build) on the same input, with the iteration counts.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_sfm_ba.py` the kernel alone (DBG_SIZES=300 restricts the sizes,
DBG_REF_CALLS=0 leaves the restatement out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sfm_ba_ref as sr
from golden import gen_sfm_ba_hp as gen
from lfvio.engine import Engine
eng = Engine(0)
CALLS, WARM = 20, 3
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "1"))
for P in [int(v) for v in os.environ.get("DBG_SIZES", "60,300,1000").split(",")]:
    sc = gen.make_scene(seed=700 + P, F=11, P=P, l=4, tracks="ragged")
    args = (sc["l"], sc["off"], sc["frame"], sc["bearing"], sc["q0"], sc["t0"], sc["X0"])
    for _ in range(WARM): out = eng.sfm_ba(*args)
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); out = eng.sfm_ba(*args); ts.append(time.perf_counter() - t)
    line = (f"F=11 P={P} M={len(sc['frame'])}: lfvio_sfm_ba median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers), "
            f"{out['num_iterations']} iterations, termination {out['termination']}, final cost {out['final_cost']:.6e}")
    if REF_CALLS:
        pb = sr.problem(sc["F"], sc["l"], sc["off"], sc["frame"], sc["bearing"])
        rs = []
        for _ in range(REF_CALLS):
            t = time.perf_counter(); ref = sr.solve(pb, sc["q0"], sc["t0"], sc["X0"]); rs.append(time.perf_counter() - t)
        line += (f"; numpy restatement median {np.median(rs)*1e3:.0f} ms, {ref['num_iterations']} iterations, final cost {ref['final_cost']:.6e}, "
                 f"largest |position - restatement's| {np.abs(out['position'] - ref['position']).max():.2e}")
    print(line)
