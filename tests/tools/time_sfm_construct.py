"""lfvio_sfm_construct at F = 11, l = 4, P in {60, 300, 1000} (40 % full tracks, the others random runs, 1 px noise; the scenes of
tests/golden/gen_sfm_chain_hp.py): median / p95 of the whole call (host buffers in / out) over 20 calls after 3 warm-up calls, beside
the numpy restatement (tests/sfm_chain_ref.py — numpy, not a tuned C++ build) on the same input.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_sfm_construct.py` the kernel alone (DBG_SIZES=300 restricts the sizes,
DBG_REF_CALLS=0 leaves the restatement out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sfm_chain_ref as cr
from golden import gen_sfm_chain_hp as gen
from lfvio.engine import Engine
eng = Engine(0)
CALLS, WARM = 20, 3
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "1"))
for P in [int(v) for v in os.environ.get("DBG_SIZES", "60,300,1000").split(",")]:
    sc = gen.make_scene(seed=700 + P, F=11, P=P, l=4, full=2 * P // 5, line=10.0)
    args = (sc["F"], sc["l"], sc["off"], sc["frame"], sc["bearing"], sc["relative_R"], sc["relative_T"])
    for _ in range(WARM): out = eng.sfm_construct(*args)
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); out = eng.sfm_construct(*args); ts.append(time.perf_counter() - t)
    line = (f"F=11 P={P} M={len(sc['frame'])}: lfvio_sfm_construct median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers), "
            f"status {out['status']}, {out['num_triangulated']} triangulated, PnP counts {out['pnp_count'].tolist()}")
    if REF_CALLS:
        rs = []
        for _ in range(REF_CALLS):
            t = time.perf_counter(); ref = cr.construct(*args); rs.append(time.perf_counter() - t)
        same = np.array_equal(out["tri_op"], ref["tri_op"]) and np.array_equal(out["pnp_count"], ref["pnp_count"])
        line += (f"; numpy restatement median {np.median(rs)*1e3:.0f} ms, status {ref['status']}, same ops {same}, "
                 f"largest |position - restatement's| {np.abs(out['position'] - np.asarray(ref['position'], np.float64)).max():.2e}")
    print(line)
