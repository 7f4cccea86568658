"""lfvio_two_view for N in {30, 150, 1000} matches, S = 100 sample sets: median / p95 of the whole call (host buffers in / out)
over 50 calls after 5 warm-up calls, beside the numpy restatement (tests/twoview_ref.py — numpy, not a tuned C++ build) on the
same inputs.  Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_two_view.py` the kernels alone
(DBG_N=150 restricts the sizes, DBG_REF_CALLS=0 leaves the restatement out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio.engine import Engine
eng = Engine(0)
S, CALLS, WARM = 100, 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "5"))
for N in [int(x) for x in os.environ.get("DBG_N", "30,150,1000").split(",")]:
    c = gen.make_case(900 + N, N, noise_px=0.3, outliers=0.1)
    s = gen.make_samples(901 + N, N, S)
    for _ in range(WARM): out = eng.two_view(c["bl"], c["br"], s)
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); out = eng.two_view(c["bl"], c["br"], s); ts.append(time.perf_counter() - t)
    rs = []
    for _ in range(REF_CALLS):
        t = time.perf_counter(); ref = tv.two_view(c["bl"], c["br"], s); rs.append(time.perf_counter() - t)
    line = f"N={N} S={S}: lfvio_two_view median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers)"
    if rs:
        same = out["best_sample"] == ref["best_sample"] and np.array_equal(out["mask"], ref["mask"])
        line += f"; numpy restatement median {np.median(rs)*1e3:.1f} ms; inliers {out['num_inliers']}, same winner and mask: {same}"
    print(line)
