"""lfvio_vi_align for F in {11, 30, 128} image frames with 20 IMU samples per span: median / p95 of the whole call (host buffers in /
out, the ctypes structures built once) over 50 calls after 5 warm-up calls, beside the numpy restatement (tests/vialign_ref.py —
numpy with a Python-loop LDL^T, not a tuned C++ build) on the same inputs.  Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/time_vi_align.py` the kernels alone (DBG_F=30 restricts the sizes,
DBG_REF_CALLS=0 leaves the restatement out)."""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import vialign_ref as va
from lfvio import abi
from lfvio.engine import Engine
eng = Engine(0)
CALLS, WARM = 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "3"))
dp = C.POINTER(C.c_double)
for F in [int(x) for x in os.environ.get("DBG_F", "11,30,128").split(",")]:
    r = va.make_regime(seed=700 + F, F=F, lengths=[20], bias=0.02, sfm_noise=(0.1, 0.005), scale=2.0, keyframe=F // 2)
    R, T = np.ascontiguousarray(r["R"].reshape(-1, 9)), np.ascontiguousarray(r["T"])
    arr, keep = (abi.ImuIntervalC * F)(), []
    for k in range(1, F):
        ba, bg, a0, g0, dts, accs, gyrs = [np.ascontiguousarray(v, dtype=np.float64) for v in r["spans"][k]]
        keep.append((dts, accs, gyrs))
        arr[k].num_samples = len(dts)
        arr[k].dt, arr[k].acc, arr[k].gyr = dts.ctypes.data_as(dp), accs.ctypes.data_as(dp), gyrs.ctypes.data_as(dp)
        for name, v in (("acc_0", a0), ("gyr_0", g0), ("linearized_ba", ba), ("linearized_bg", bg)):
            setattr(arr[k], name, (C.c_double * 3)(*v))
    vin, out, x = abi.ViAlignInC(), abi.ViAlignOutC(), np.zeros(3 * F)
    vin.num_frames, vin.R, vin.T, vin.span = F, R.ctypes.data_as(dp), T.ctypes.data_as(dp), arr
    vin.noise, vin.tic, vin.g_norm = (C.c_double * 4)(*r["noise"]), (C.c_double * 3)(*r["tic"]), r["G"]
    call = lambda: eng.lib.lfvio_vi_align(eng.ctx, C.byref(vin), C.byref(out), x.ctypes.data_as(dp), None)
    for _ in range(WARM): assert call() == 0
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
    rs = []
    for _ in range(REF_CALLS):
        t = time.perf_counter(); ref = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"]); rs.append(time.perf_counter() - t)
    line = f"F={F} x 20 samples: lfvio_vi_align median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers), status {out.status}"
    if rs:
        line += f"; numpy restatement median {np.median(rs)*1e3:.0f} ms; s {out.s:.9g} vs {ref['s']:.9g}"
    print(line)
