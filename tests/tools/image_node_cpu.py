"""The image route on the CPU alone: a make_image_stream recording through the RESTATED node — node_ref.Gate around
tests/track_frame_ref.Frame, no device — then the derived feature recording through the host sources over the CPU checker
(oracle.binding.build_host_oracle).  Prints the rows of every message, the replay's stats and the ATE: the conditions of
tests/test_image_replay.py's second test were chosen so that this script meets them before the device is asked.

    python tests/tools/image_node_cpu.py [seed] [frames] [scale]        (defaults 0 36 4: the test's recording; about 10 s)"""
import os, struct, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lf-vio_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import ate
import node_ref as nr
import track_frame_ref as tf
from lfvio import engine, trace
from lfvio.host import HostEstimator
from oracle import binding

seed, n_frames, scale = (int(a) for a in (sys.argv[1:] + ["0", "36", "4"][len(sys.argv) - 1:]))
MAX_CNT, MIN_DIST, S, SEED = (80, 12, 100, 77) if scale > 1 else (150, 30, 100, 77)
d = tempfile.mkdtemp(prefix="image_node_cpu_")
src, dst, traj = os.path.join(d, "images.lfvt"), os.path.join(d, "tracked.lfvt"), os.path.join(d, "traj.txt")
made = trace.make_image_stream(src, seed=seed, n_frames=n_frames, scale=scale)
fr = tf.Frame(base_mask=engine.annulus_mask(made["width"], made["height"], *made["annulus"]))
gate, rng, msgs, t0 = nr.Gate(10), np.random.RandomState(SEED), {}, time.time()
for k, (t, img) in enumerate(trace.read_trace(src)["raw_images"]):
    what = gate.on_stamp(t)
    if what != nr.TRACKED:
        print(k, "dropped" if what == nr.DROP else "restart")
        continue
    pub = gate.publish
    words = rng.randint(0, 2 ** 32, size=(S, 8), dtype=np.uint32) if pub else None
    r = fr.read(img, t, made["camera"], publish=pub, words=words, max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
    what = gate.after_frame()
    rows = nr.rows_from_table(r["pts"], r["ids"], r["track_cnt"], r["un_pts_3d"], r["velocity_3d"])
    print(k, {nr.TRACKED: "tracked only", nr.FIRST_PUBLICATION: "first publication skipped", nr.PUBLISHED: "published"}[what], "points", len(r["ids"]),
          "rows", len(rows), f"{time.time() - t0:.0f} s", flush=True)
    if what == nr.PUBLISHED:
        msgs[k] = (t, rows)
# the derived recording: every image replaced by its message, the rest copied
w, k = trace.TraceWriter(dst), 0
with open(src, "rb") as f:
    f.read(8)
    while True:
        h = f.read(8)
        if len(h) < 8:
            break
        kind, nb = struct.unpack("<II", h)
        p = f.read(nb)
        if kind != trace.REC_IMAGE:
            w._rec(kind, p)
            continue
        if k in msgs:
            w._rec(trace.REC_FEATURES, struct.pack("<dI", msgs[k][0], len(msgs[k][1])) + msgs[k][1].astype("<f4").tobytes())
        k += 1
w.close()
he = HostEstimator(binding.build_host_oracle())
he.clear_state(); he.set_min_parallax(10.0); he.set_solver_time(0.0)
rc, st = he.replay(dst, traj)
he.close()
print("messages", len(msgs), "rows", min(len(r) for _, r in msgs.values()), "to", max(len(r) for _, r in msgs.values()))
print("replay on the CPU checker: rc", rc, st)
print("ATE", ate.ate(traj, dst) if st["poses"] >= 3 else None)
