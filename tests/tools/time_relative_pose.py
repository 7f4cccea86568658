"""lfvio_relative_pose at P = 10 pairs, S = 100 sample sets, N in {30, 150, 1000} matches per pair: median / p95 of the whole call
(host buffers in / out) over 50 calls after 5 warm-up calls, beside (a) P sequential Engine.two_view calls on the same pairs — what
the library could do before the entry existed — and (b) the numpy restatement (tests/relpose_ref.py — numpy, not a tuned C++ build).
Then the ATE of a self-initialized replay (Config::self_relative_pose, no record of any kind) beside the ATE of the same recording
with ONE relative pose record made from the truth.  Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_relative_pose.py`
the kernels alone (DBG_N=150 restricts the sizes, DBG_REF_CALLS=0 leaves the restatement out, DBG_ATE=0 the replays)."""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import relpose_ref as rp
from golden import gen_twoview_hp as gen
from lfvio.engine import Engine
eng = Engine(0)
P, S, CALLS, WARM = 10, 100, 50, 5
REF_CALLS = int(os.environ.get("DBG_REF_CALLS", "3"))
for N in [int(x) for x in os.environ.get("DBG_N", "30,150,1000").split(",")]:
    cs = [gen.make_case(900 + N + p, N, noise_px=0.3, outliers=0.1, baseline=0.3 + 0.05 * p) for p in range(P)]
    off = (N * np.arange(P + 1)).astype(np.int32)
    bl, br = np.vstack([c["bl"] for c in cs]), np.vstack([c["br"] for c in cs])
    sm = np.stack([gen.make_samples(950 + N + p, N, S) for p in range(P)]).astype(np.int32)
    for _ in range(WARM): out = eng.relative_pose(off, bl, br, sm)
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter(); out = eng.relative_pose(off, bl, br, sm); ts.append(time.perf_counter() - t)
    for _ in range(WARM): seq = [eng.two_view(c["bl"], c["br"], sm[p]) for p, c in enumerate(cs)]
    qs = []
    for _ in range(CALLS):
        t = time.perf_counter(); seq = [eng.two_view(c["bl"], c["br"], sm[p]) for p, c in enumerate(cs)]; qs.append(time.perf_counter() - t)
    rs = []
    for _ in range(REF_CALLS):
        t = time.perf_counter(); ref = rp.relative_pose(off, bl, br, sm); rs.append(time.perf_counter() - t)
    same_tv = all(q["gate"] == 0 and q["best_sample"] == t_["best_sample"] and q["E"].tobytes() == t_["E"].tobytes() for q, t_ in zip(out["pair"], seq))
    line = (f"P={P} N={N} S={S}: lfvio_relative_pose median {np.median(ts)*1e6:.0f} us, p95 {np.percentile(ts, 95)*1e6:.0f} us per call (host buffers); "
            f"{P} sequential lfvio_two_view calls median {np.median(qs)*1e6:.0f} us, p95 {np.percentile(qs, 95)*1e6:.0f} us, same bits: {same_tv}")
    if rs:
        same = out["l"] == ref["l"] and all(q["gate"] == r["gate"] and q["best_sample"] == r["best_sample"] for q, r in zip(out["pair"], ref["pair"]))
        line += f"; numpy restatement median {np.median(rs)*1e3:.1f} ms; l = {out['l']}, same l, gates and winners: {same}"
    print(line)
eng.close()

if os.environ.get("DBG_ATE", "1") != "0":
    import __graft_entry__ as ge
    ge.build()
    import ate
    from lfvio import abi, trace
    from lfvio.host import HostEstimator
    from test_pnp_host import fresh, raw_records
    from test_sfm_construct_host import rename_returning_ids
    d = tempfile.mkdtemp()
    src, bare, rec = os.path.join(d, "src.lfvt"), os.path.join(d, "bare.lfvt"), os.path.join(d, "rec.lfvt")
    s = trace.make_stream(src, seed=3, n_frames=30, pixel_noise=0.1)
    s["images"] = rename_returning_ids(s["images"])
    W = abi.WINDOW_SIZE
    by = {t: (Pp, R) for t, Pp, R, _ in s["truth"]}
    kf = [im[0] for im in s["images"][:W + 1]]  # the first full window: eleven keyframes while nothing slides a non-keyframe out
    wb, wr, k = trace.TraceWriter(bare), trace.TraceWriter(rec), 0
    for kind, payload in raw_records(src):
        if kind == trace.REC_BOOTSTRAP:
            continue
        if kind == trace.REC_FEATURES:
            a = np.frombuffer(payload[12:], dtype="<f4").reshape(-1, 9).copy()
            a[:, 3] = s["images"][k][1]
            payload = payload[:12] + a.tobytes()
            if k == W:
                wr.relative_pose(kf[-1], 0, *trace.relative_pose_from_truth([by[t][0] for t in kf], [by[t][1] for t in kf], 0))
            k += 1
        wb._rec(kind, payload), wr._rec(kind, payload)
    wb.close(), wr.close()
    host = HostEstimator()
    host.set_ransac(20241, 100)
    for name, path, on in (("self-initialized (no record)", bare, True), ("one relative pose record from the truth (l = 0)", rec, False)):
        host.set_self_relative_pose(on)
        fresh(host)
        jp = os.path.join(d, "traj.txt")
        rc, st = host.replay(path, jp)
        r = ate.ate(jp, src) if rc == 0 and st["poses"] >= 3 else None
        print(f"replay, {name}: rc {rc}, {st['poses']} poses of {st['images']} images, failures {st['failures']}; "
              + (f"ATE rmse {r['rmse']:.4f} m, mean {r['mean']:.4f} m, max {r['max']:.4f} m over {r['n']} poses" if r else "no trajectory"))
    host.set_self_relative_pose(False)
    host.close()
