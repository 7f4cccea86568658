"""lfvio_pnp for (F, n) in {(1, 30), (20, 150), (128, 150), (128, 1000)} — F frames of n correspondences each: median / p95 of the
whole call (host buffers in / out) over 50 calls after 5 warm-up calls, beside the numpy restatement (tests/pnp_ref.py — numpy,
not a tuned C++ build) on the same inputs.  Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_pnp.py` the kernel
alone (DBG_SIZES=20x150 restricts the sizes, DBG_REF_CALLS=0 leaves the restatement out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pnp_ref as pr
from golden import gen_pnp_hp as gen
from lfvio.engine import Engine
eng = Engine(0)
CALLS, WARM = 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "2"))
for F, n in [tuple(int(v) for v in x.split("x")) for x in os.environ.get("DBG_SIZES", "1x30,20x150,128x150,128x1000").split(",")]:
    cases = [gen.make_case(900 + 131 * f + n, n, noise_px=1.0, f32=True) for f in range(F)]
    off = (np.arange(F + 1) * n).astype(np.int32)
    pw, us = np.concatenate([c["pw"] for c in cases]), np.concatenate([c["us"] for c in cases])
    for _ in range(WARM): out = eng.pnp(off, pw, us)
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); out = eng.pnp(off, pw, us); ts.append(time.perf_counter() - t)
    rs = []
    for _ in range(REF_CALLS):
        t = time.perf_counter(); ref = pr.pnp(off, pw, us); rs.append(time.perf_counter() - t)
    line = f"F={F} n={n}: lfvio_pnp median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers)"
    if rs:
        d = max(np.abs(o["R"] - r["R"]).max() for o, r in zip(out, ref))
        line += f"; numpy restatement median {np.median(rs)*1e3:.1f} ms; largest |R - restatement's R| {d:.2e}, all status 0: {all(o['status'] == 0 for o in out)}"
    print(line)
