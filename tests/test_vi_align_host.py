"""Initialization from SfM poses on the host: all_image_frame, SfM records (trace type 7), WindowEstimator::visualInitialAlign.

CPU: the record type round-trips through TraceWriter / read_trace / Trace::load and a trace without it reads as before; over the
oracle-backed C-ABI (which has no lfvio_vi_align) the attempt reports LFVIO_ERR_DEVICE; the image-frame list follows the
bookkeeping of estimator.cpp:137-140 and :1051-1067, restated here, over 20 images with non-keyframes.

GPU: the host against the numpy restatement (tests/vialign_ref.py) on the host's own inputs; a 60-image recording with an SfM
record instead of its bootstrap record replayed to the end; the reboot recording of test_flow.py with SfM records; records
that are not applied (a missing stamp, a failing gate).

Measured values and bars are in the docstrings of the tests.
"""
import os
import sys

import numpy as np
import pytest

import flow_ref
import vialign_ref as va
from lfvio import abi, synth, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
W = abi.WINDOW_SIZE


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as ge

    ge.build()
    from lfvio.host import HostEstimator

    h = HostEstimator()
    yield h
    h.close()


def fresh(host, parallax_px=10.0):
    """A cleared estimator with the recording's extrinsic and td configured (an SfM record carries none) -> its alignment counters."""
    host.set_extrinsic(synth.TIC, synth.RIC)
    host.set_td(synth.TD0)
    host.clear_state()
    host.set_min_parallax(parallax_px)
    return host.vi_align_counts()


def since(host, c0):
    c = host.vi_align_counts()
    return c[0] - c0[0], c[1] - c0[1]


def image_arrays(img):
    stamp, ids, xyz, uv, vel = img
    return stamp, ids, np.concatenate([xyz, uv.astype(np.float32).astype(np.float64), vel], axis=1)


def sfm_recording(tmp_path, seed=3, n_frames=60, **kw):
    src, dst = str(tmp_path / f"boot{seed}.lfvt"), str(tmp_path / f"sfm{seed}.lfvt")
    s = trace.make_stream(src, seed=seed, n_frames=n_frames, **{k: v for k, v in kw.items() if k in ("restart_at", "spike_at")})
    recs = trace.bootstraps_to_sfm(src, dst, **{k: v for k, v in kw.items() if k not in ("restart_at", "spike_at")})
    return src, dst, s, recs


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_sfm_records_round_trip(host, tmp_path):
    """TraceWriter.sfm -> read_trace and Trace::load give the record back; a recording without one reads as before."""
    src, dst, s, recs = sfm_recording(tmp_path, seed=7, n_frames=24, keyframe=2, scale=3.0)
    a, b = trace.read_trace(src), trace.read_trace(dst)
    assert a["sfms"] == [] and len(a["bootstraps"]) == 1 and len(b["bootstraps"]) == 0
    assert [k for k in a["order"] if k != trace.REC_BOOTSTRAP] == [k for k in b["order"] if k != trace.REC_SFM]
    assert np.array_equal(a["imu"], b["imu"]) and np.array_equal(a["truth"], b["truth"]) and len(a["images"]) == len(b["images"])
    assert len(b["sfms"]) == 2 and b["sfms"][1]["at_image"] == 10 and len(b["sfms"][1]["stamps"]) == 12
    r = b["sfms"][0]
    assert r["at_image"] == 10 and r["stamp"] == b["images"][10][0] and len(r["stamps"]) == 11
    assert np.array_equal(r["stamps"], [t for t, _ in b["images"][:11]])
    assert np.array_equal(r["R"], recs[0]["R"]) and np.array_equal(r["T"], recs[0]["T"])
    assert np.allclose(r["R"][2], synth.RIC.T, atol=1e-12) and np.allclose(r["T"][2], 0, atol=1e-12)  # the camera frame of image 2: R = R_c<-b
    # the same through the C++ loader
    import ctypes as C

    L = host.L
    st, fr = np.zeros(4), np.zeros(4, dtype=np.int32)
    R, T = np.zeros((11, 9)), np.zeros((11, 3))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.lfvio_host_trace_sfms.argtypes = [C.c_char_p, C.c_int, dp, ip, dp, dp, C.c_int]
    n = L.lfvio_host_trace_sfms(dst.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), R.ctypes.data_as(dp), T.ctypes.data_as(dp), 11)
    assert n == 2 and st[0] == r["stamp"] and fr[0] == 11 and fr[1] == 12
    assert np.array_equal(R.reshape(11, 3, 3), r["R"]) and np.array_equal(T, r["T"])
    assert L.lfvio_host_trace_sfms(src.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), None, None, 0) == 0
    # ... and from a bag: the SfM hook's std_msgs/Float64MultiArray (stamp, F, F x 13) through tools/bag_to_lfvt.py, bit for bit
    import bag_to_lfvt
    from lfvio import rosmsg

    for comp in ("none", "bz2"):
        bp, op = str(tmp_path / f"run_{comp}.bag"), str(tmp_path / f"from_bag_{comp}.lfvt")
        bw = rosmsg.BagWriter(bp, compression=comp, chunk_messages=50)
        ii = im = isf = seq = 0
        for kind in b["order"]:
            seq += 1
            if kind == trace.REC_IMU:
                m = b["imu"][ii]
                ii += 1
                bw.write("/imu0", "sensor_msgs/Imu", m[0] + 1e-4, rosmsg.ser_imu(seq, m[0], m[1:4], m[4:7]))
            elif kind == trace.REC_FEATURES:
                t, arr = b["images"][im]
                im += 1
                bw.write("/feature_tracker/feature", "sensor_msgs/PointCloud", t + 2e-2, rosmsg.ser_pointcloud(seq, t, arr))
            elif kind == trace.REC_SFM:
                q = b["sfms"][isf]
                isf += 1
                body = np.concatenate([q["stamps"][:, None], q["R"].reshape(-1, 9), q["T"]], axis=1)
                bw.write("/vins_estimator/lfvt_sfm", "std_msgs/Float64MultiArray", 0.0,
                         rosmsg.ser_f64_array(np.concatenate([[q["stamp"], len(body)], body.ravel()])))
        bw.close()
        cnt = bag_to_lfvt.convert(bp, op)
        assert cnt == dict(imu=len(b["imu"]), images=len(b["images"]), restarts=0, bootstraps=0, other=0, sfms=2)
        got = trace.read_trace(op)
        assert got["order"] == [k for k in b["order"] if k != trace.REC_TRUTH] and len(got["sfms"]) == 2
        for x, y in zip(got["sfms"], b["sfms"]):
            assert x["stamp"] == y["stamp"] and x["at_image"] == y["at_image"]
            assert all(np.array_equal(x[k], y[k]) for k in ("stamps", "R", "T"))
        assert L.lfvio_host_trace_sfms(op.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), R.ctypes.data_as(dp), T.ctypes.data_as(dp), 11) == 2
        assert np.array_equal(R.reshape(11, 3, 3), r["R"]) and np.array_equal(T, r["T"])
    # a message whose length is not 2 + 13 F is refused by the converter
    bw = rosmsg.BagWriter(str(tmp_path / "short.bag"))
    bw.write("/vins_estimator/lfvt_sfm", "std_msgs/Float64MultiArray", 0.0, rosmsg.ser_f64_array(np.concatenate([[1.0, 2.0], np.zeros(25)])))
    bw.close()
    with pytest.raises(ValueError):
        bag_to_lfvt.convert(str(tmp_path / "short.bag"), str(tmp_path / "short.lfvt"))
    # a record whose length does not match its frame count is refused like any malformed record
    raw = open(dst, "rb").read()
    bad = str(tmp_path / "bad.lfvt")
    open(bad, "wb").write(raw[:8] + (7).to_bytes(4, "little") + (20).to_bytes(4, "little") + b"\0" * 8 + (3).to_bytes(4, "little") + b"\0" * 8)
    assert L.lfvio_host_trace_sfms(bad.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), None, None, 0) == -1


def test_oracle_abi_reports_err_device(oracle, tmp_path):
    """The CPU checker's C-ABI has no lfvio_vi_align: the attempt reports LFVIO_ERR_DEVICE (the replay stops on it, -2) and the
    estimator is still initializing with its window slid."""
    from oracle import binding as ob

    from lfvio.host import HostEstimator

    src, dst, s, recs = sfm_recording(tmp_path, seed=7, n_frames=24)
    h = HostEstimator(ob.build_host_oracle())
    fresh(h)
    rc, st = h.replay(dst)
    assert rc == -2 and st["last_status"] == -2 and st["bootstraps"] == 0 and st["poses"] == 0, st
    fl = h.flow()
    assert fl["solver_flag"] == 0 and fl["frame_count"] == W and fl["sum_of_back"] + fl["sum_of_front"] == 1
    assert h.vi_align_counts() == (0, 0)
    lv = h.last_vi_align()
    assert not lv["called"] and lv["rc"] == -2 and len(lv["stamps"]) == 11
    # the recording with its bootstrap record replays on that stack as it always did
    h.clear_state()
    rc, st = h.replay(src)
    assert rc == 0 and st["bootstraps"] == 1 and st["poses"] == st["images"] - 10
    h.close()


@pytest.mark.parametrize("px", [10.0, 40.0])
def test_image_frame_list_bookkeeping(host, tmp_path, px):
    """all_image_frame over 20 images without any initialization record: one entry per image with the samples since the previous
    image (none for the first: no integration before frame_count != 0), a MARGIN_OLD slide erases everything up to and including
    Headers[0] (estimator.cpp:1051-1067), MARGIN_SECOND_NEW keeps the entry; reset() clears the list."""
    p = str(tmp_path / "s7.lfvt")
    s = trace.make_stream(p, seed=7, n_frames=24)
    rd = trace.read_trace(p)
    fresh(host, px)
    ref = flow_ref.Flow(px / 160.0)
    want, kinds = [], set()
    for stamp, idx, calls in flow_ref.sync(rd["imu"], [(im[0], None) for im in s["images"]], lambda: synth.TD0):
        if idx >= 20:
            break
        for dt, a, g in calls:
            host.process_imu(dt, a, g)
            ref.process_imu(dt, a, g)
        full, t0, n = ref.frame_count == W, ref.Headers[0], len(calls) if ref.frame_count != 0 else 0
        _, ids, pts = image_arrays(s["images"][idx])
        assert host.process_image(stamp, ids, pts) == 0
        ref.process_image(ids, pts, stamp)
        want.append((stamp, n))
        if full and ref.marg_old:
            want = [e for e in want if e[0] > t0]
        if full:
            kinds.add(bool(ref.marg_old))
        st, ns = host.image_frames()
        assert list(st) == [e[0] for e in want] and list(ns) == [e[1] for e in want], idx
    assert len(want) >= W and (px < 20 or kinds == {True, False})
    if px > 20:
        assert len(want) > W  # non-keyframes stay in the list
    host.clear_state()
    assert len(host.image_frames()[0]) == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
def fill_window(host, s, rd, n_images=12, px=10.0, first=0, ref=None):
    """Feed images [first, n_images) without any record (first = 0: from a cleared estimator); ref: a flow_ref.Flow fed alongside."""
    c0 = fresh(host, px) if first == 0 else None
    for stamp, idx, calls in flow_ref.sync(rd["imu"], [(im[0], None) for im in s["images"]], lambda: synth.TD0):
        if idx >= n_images:
            break
        if idx < first:
            continue
        for dt, a, g in calls:
            host.process_imu(dt, a, g)
            if ref is not None:
                ref.process_imu(dt, a, g)
        _, ids, pts = image_arrays(s["images"][idx])
        assert host.process_image(stamp, ids, pts) == 0
        if ref is not None:
            ref.process_image(ids, pts, stamp)
    return c0


def truth_sfm(s, stamps, **kw):
    by = {t: (P, R) for t, P, R, _ in s["truth"]}
    return trace.sfm_from_truth(stamps, [by[t][0] for t in stamps], [by[t][1] for t in stamps], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("px", [10.0, 40.0])
def test_host_state_equals_the_restatement(host, tmp_path, px):
    """visualInitialAlign() alone on a full window (40 px: with non-keyframes in the list, so the kv indexing of :409-418 matters):
    last_vi_align()'s inputs through the restatement give the same status and the same window state.

    Ps, Rs, Vs, Bgs, g: within 16 x the largest change of the restatement's state when EVERY input — R, T and the samples acc, gyr,
    acc_0, gyr_0 of every span — moves by one ulp up or down at random, over three trials (the construction of test_exrot_host.py).
    Depths, per feature id: the device's triangulation on the SfM poses (tic = 0, configured ric) times the device's s against
    np_ref.triangulate on the same poses times the same s (window_depths_np: estimator.cpp:389-425), in the unit of
    test_feature_hp.py, eps sigma_1/sigma_4 of the landmark's system relative to the depth; bar 352 + 22 = 374, that file's bar for
    the device against a double-precision restatement on a window (16 x the restatements' worst against 50 digits, plus that
    worst); the fallbacks to init_depth are the same tracks on both sides and equal 5 s exactly.
    Measured on an MI355X (host - restatement / bar): 10 px Ps 2.7e-13 / 2.8e-12, Rs 2.1e-14 / 7.5e-13, Vs 3.4e-13 / 3.5e-12, Bgs 9.5e-18 / 3.0e-16, g 2.1e-15 / 2.8e-14, depths 14.2 / 374;
    40 px Ps 1.5e-13 / 1.7e-12, Rs 9.3e-16 / 1.3e-13, Vs 1.5e-13 / 1.8e-12, Bgs 3.7e-17 / 4.2e-16, g 1.8e-15 / 2.8e-14, depths 1.53 / 374."""
    from lfvio.engine import Engine  # noqa: F401  (torch first: the ROCm wheel brings its own HIP runtime)

    p = str(tmp_path / "s3.lfvt")
    s = trace.make_stream(p, seed=3, n_frames=30)
    rd = trace.read_trace(p)
    import copy

    flow = flow_ref.Flow(px / 160.0)  # the track table restated: which observations each track holds when the alignment runs
    c0 = fill_window(host, s, rd, n_images=14, px=px, ref=flow)
    host.set_stop_after_align(True)
    try:
        for n in range(14, 20):  # (initialization is attempted when more than 0.1 s have passed since the last attempt: every other image)
            before = host.state()
            tracks = copy.deepcopy(flow)  # ... with this image's observations added and nothing slid yet
            _, ids_n, pts_n = image_arrays(s["images"][n])
            tracks.add_feature_check_parallax(tracks.frame_count, ids_n, pts_n)
            stamps = list(host.image_frames()[0]) + [s["images"][n][0]]  # the list as the next image will find it
            host.set_sfm(*truth_sfm(s, stamps, keyframe=3, scale=2.5, rot_noise_deg=0.1, pos_noise=0.005, seed=11))
            fill_window(host, s, rd, n_images=n + 1, px=px, first=n, ref=flow)
            if since(host, c0) != (0, 0):
                break
    finally:
        host.set_stop_after_align(False)
    assert px < 20 or len(stamps) > W + 1
    kf_stamps = host.buffers()["stamps"]
    assert since(host, c0) == (1, 1) and host.flow()["solver_flag"] == 0
    lv = host.last_vi_align()
    assert lv["called"] and lv["rc"] == 0 and lv["out"]["status"] == 0 and np.array_equal(lv["stamps"], stamps)
    a = (lv["R"], lv["T"], lv["spans"], lv["noise"], lv["tic"], lv["G"])
    ref = va.align_np(*a)
    assert ref["status"] == 0
    want = va.window_state_np(ref, lv["R"], lv["T"], lv["stamps"], kf_stamps, lv["tic"], before["Bgs"])
    got = host.state()
    got["g"] = host.gravity()
    # the bar: one ulp on every input at once, through the restatement's whole chain
    change = {k: 0.0 for k in want}
    for trial in range(3):
        rng = np.random.default_rng(trial)
        pt = lambda v: np.nextafter(v, np.where(rng.random(np.shape(v)) < 0.5, -np.inf, np.inf))
        R_, T_ = pt(lv["R"]), pt(lv["T"])
        spans_ = [None] + [(sp[0], sp[1], pt(sp[2]), pt(sp[3]), sp[4], pt(sp[5]), pt(sp[6])) for sp in lv["spans"][1:]]
        w2 = va.window_state_np(va.align_np(R_, T_, spans_, *a[3:]), R_, T_, lv["stamps"], kf_stamps, lv["tic"], before["Bgs"])
        for k in want:
            change[k] = max(change[k], np.abs(w2[k] - want[k]).max())
    for k in want:
        d = np.abs(got[k] - want[k]).max()
        print(f"px {px} {k}: host - restatement {d:.3g}, one-ulp change {change[k]:.3g}, bar {16 * change[k]:.3g}")
        assert d <= 16 * change[k], k
    assert np.array_equal(got["Bas"], before["Bas"])
    # depths, per feature id
    ids, start, cnt, depth = host.features()
    solvable = (cnt >= 2) & (start < W - 2)
    assert np.isfinite(depth).all() and np.all(depth[~solvable] == -1.0)
    s_dev = lv["out"]["s"]
    assert [list(a) for a in zip(ids, start, cnt)] == [[f[0], f[1], len(f[2])] for f in tracks.feature]
    want_d, cond = window_depths_np(lv, kf_stamps, [f for f in tracks.feature if len(f[2]) >= 2 and f[1] < W - 2], s_dev)
    fb = want_d == 5.0 * s_dev
    assert np.array_equal(depth[solvable] == 5.0 * s_dev, fb), "another set of tracks falls back to init_depth"
    m = np.abs(depth[solvable] - want_d) / np.abs(want_d) / (va.EPS * cond)
    print(f"px {px}: {int(solvable.sum())} solvable tracks, {int(fb.sum())} at init_depth x s; depths worst {m.max():.3g} eps sigma1/sigma4 (bar 374)")
    assert m.max() <= 374.0, (ids[solvable][m.argmax()], m.max())


def window_depths_np(lv, kf_stamps, tracks, s_scale):
    """estimator.cpp:389-425 restated with tests/np_ref.py for tracks [feature id, start frame, [bearings]] (flow_ref's table: as in
    the reference, observation k of a track counts as seen in frame start + k) of the window whose keyframes carry kf_stamps:
    triangulated on the SfM poses of those keyframes with tic = 0 and the configured ric, init_depth where the result is negative,
    everything x s_scale.  -> (depths, sigma_1 / sigma_4 of every track's system)."""
    import np_ref

    idx = [int(np.flatnonzero(np.asarray(lv["stamps"]) == t)[0]) for t in kf_stamps]
    Ps, Rs = lv["T"][idx], lv["R"][idx]
    ids, start, off, pts = [], [], [0], []
    for fid, f0, obs in tracks:
        ids.append(fid), start.append(f0), pts.extend(np.asarray(o, float) for o in obs), off.append(len(pts))
    pts = np.array(pts)
    d = np_ref.triangulate(start, off, pts, Ps, Rs, np.zeros(3), synth.RIC, np.full(len(ids), -1.0), 5.0)
    cond = np.zeros(len(ids))
    for l in range(len(ids)):
        i0, rows = int(start[l]), []
        R0 = Rs[i0] @ synth.RIC
        for o in range(off[l + 1] - off[l]):
            R1 = Rs[i0 + o] @ synth.RIC
            R = R0.T @ R1
            P = np.hstack([R.T, (-R.T @ (R0.T @ (Ps[i0 + o] - Ps[i0])))[:, None]])
            f = pts[off[l] + o] / np.linalg.norm(pts[off[l] + o])
            rows += [f[0] * P[2] - f[2] * P[0], f[1] * P[2] - f[2] * P[1]]
        sv = np.linalg.svd(np.array(rows), compute_uv=False)
        cond[l] = sv[0] / sv[3]
    return d * s_scale, cond


@pytest.mark.gpu
def test_sfm_recording_replays_to_the_end(host, tmp_path, scale=2.5):
    """The 60-image recording of test_flow's end-to-end test with an SfM record (noise-free, the camera frame of image 4, positions
    divided by 2.5) instead of its bootstrap record: no bootstrap, one alignment, a pose per image after the tenth.  Scale, gravity
    direction and gyroscope bias against the recording's truth at 2 x the restatement's own error on the same input (measured:
    scale 2.693e-02, gravity direction 2.470e-04 rad, gyroscope bias 1.574e-03 rad/s on both sides, equal to the printed digits).

    The ATE equals, to the 1 % of the other replay comparisons, that of the numpy restatement's aligned state pushed in through
    set_bootstrap.  That state is ALL of what estimator.cpp:380-437 leaves: Ps, Rs, Vs, Bgs, g AND the depths (:389-425: triangulated
    on the SfM poses, init_depth where negative, then every solvable depth x s), restated with np_ref.triangulate and handed over
    by feature id — a deliberate extension of the comparison as the issue words it: a Bootstrap may carry depths for this.  Without the depths the two routes do not start from the same window and the comparison fails by 2.4 %
    (measured: SfM route 0.02912 m against 0.02983 m; 4.2 % inside the whole suite): 18 of the 209 solvable tracks fall back to
    init_depth and start at 5 s = 12.4 m on the SfM route but at 5 m when the bootstrap path triangulates them on the metric state,
    and the linear triangulation itself is not invariant to the scale of the translations.  Shown by leaving the fallback tracks
    unscaled in a trial build (0.02975 against 0.02983 m) and by a recording without pixel noise, where no track falls back
    (0.002743 m on both routes).  The figure without depths is printed beside the others."""
    import ate
    from lfvio.engine import Engine  # noqa: F401

    src, dst, s, recs = sfm_recording(tmp_path, seed=3, n_frames=60, keyframe=4, scale=scale)
    jp = {k: str(tmp_path / f"traj_{k}.txt") for k in ("sfm", "np", "np_nodepth", "boot")}
    c0 = fresh(host)
    rc, st = host.replay(dst, jp["sfm"])
    assert rc == 0 and st["last_status"] == 0 and st["failures"] == 0 and st["bootstraps"] == 0, st
    assert since(host, c0) == (1, 1) and st["images"] in (59, 60) and st["poses"] == st["images"] - 10
    lv = host.last_vi_align()
    a = (lv["R"], lv["T"], lv["spans"], lv["noise"], lv["tic"], lv["G"])
    ref = va.align_np(*a)
    out = lv["out"]
    # against the truth: the device's error is the restatement's (mid-point integration is not exact; measured on the CPU here)
    Rl = s["truth"][4][2] @ synth.RIC
    g_true = Rl.T @ np.array([0.0, 0.0, synth.G_NORM])
    ang = lambda g: np.arccos(np.clip(g @ g_true / np.linalg.norm(g) / np.linalg.norm(g_true), -1, 1))
    errs = {"scale": (abs(out["s"] - scale), abs(ref["s"] - scale)), "gravity direction": (ang(out["g"]), ang(ref["g"])),
            "gyroscope bias": (np.linalg.norm(out["delta_bg"] - s["scene"].bg), np.linalg.norm(ref["delta_bg"] - s["scene"].bg))}
    for k, (dev, rst) in errs.items():
        print(f"{k}: device {dev:.3e}, restatement {rst:.3e}")
        assert dev <= 2.0 * rst, k
    # the restatement's aligned state through the existing bootstrap path, on the same recording without any record
    none = str(tmp_path / "none.lfvt")
    wtr = trace.TraceWriter(none)
    for kind, payload in raw_records(src):
        if kind != trace.REC_BOOTSTRAP:
            wtr._rec(kind, payload)
    wtr.close()
    kf_stamps = lv["stamps"][-(W + 1):] if len(lv["stamps"]) == W + 1 else None
    assert kf_stamps is not None  # the first full window: eleven frames, all keyframes of the window
    want = va.window_state_np(ref, lv["R"], lv["T"], lv["stamps"], kf_stamps, lv["tic"], np.zeros((W + 1, 3)))
    flow = flow_ref.Flow(10.0 / 160.0)  # the track table of the first full window, restated (nothing has slid yet)
    for f, t in enumerate(kf_stamps):
        _, ids_f, pts_f = image_arrays({im[0]: im for im in s["images"]}[t])
        flow.add_feature_check_parallax(f, ids_f, pts_f)
    trk = [f for f in flow.feature if len(f[2]) >= 2 and f[1] < W - 2]
    dep_ids = np.array([f[0] for f in trk])
    dep, _ = window_depths_np(lv, kf_stamps, trk, ref["s"])
    for key, kw in (("np", dict(depth_ids=dep_ids, depths=dep)), ("np_nodepth", {})):
        fresh(host)
        host.set_bootstrap(want["Ps"], want["Rs"], want["Vs"], np.zeros((W + 1, 3)), want["Bgs"], want["g"], **kw)
        rc, st2 = host.replay(none, jp[key])
        assert rc == 0 and st2["poses"] == st["poses"]
    fresh(host)
    rc, st3 = host.replay(src, jp["boot"])
    assert rc == 0 and st3["bootstraps"] == 1
    e = {k: ate.ate(jp[k], src)["rmse"] for k in jp}
    print(f"ATE: SfM route {e['sfm']:.5f} m, restatement's state through set_bootstrap {e['np']:.5f} m (without its depths {e['np_nodepth']:.5f} m), "
          f"bootstrap record {e['boot']:.5f} m; {int(np.sum(dep == 5.0 * ref['s']))} of {len(dep)} tracks at init_depth x s")
    assert e["sfm"] < 0.05  # the bar of test_flow's end-to-end test on this recording
    assert abs(e["sfm"] / e["np"] - 1.0) < 0.01, e


def raw_records(path):
    import struct

    with open(path, "rb") as f:
        f.read(8)
        while True:
            h = f.read(8)
            if len(h) < 8:
                return
            kind, n = struct.unpack("<II", h)
            yield kind, f.read(n)


@pytest.mark.gpu
def test_sfm_reboots_mid_recording(host, tmp_path):
    """test_flow's reboot recording (restart message before image 22, accelerometer spike before image 45) with SfM records: one
    restart, one failure, three alignments, no bootstrap; records stamped before a reboot are skipped."""
    import ate
    from lfvio.engine import Engine  # noqa: F401

    src, dst, s, recs = sfm_recording(tmp_path, seed=9, n_frames=70, restart_at=22, spike_at=45, keyframe=1, scale=0.5)
    assert len(recs) == 3
    jp = str(tmp_path / "traj.txt")
    c0 = fresh(host)
    rc, st = host.replay(dst, jp)
    assert rc == 0 and st["last_status"] == 0, st
    assert st["restarts"] == 1 and st["failures"] == 1 and st["bootstraps"] == 0 and since(host, c0) == (3, 3), (st, since(host, c0))
    assert st["poses"] == st["images"] - 30 - 1, st
    # which record each alignment consumed: bootstraps_to_sfm writes two per initialization, for images k and k + 1 (10 / 11, 32 /
    # 33, 56 / 57).  The first pose of each run is the alignment image: the first two runs take the FIRST record of their pair; after
    # the failureDetection() reboot the window is full one image later than make_stream's bootstrap record assumes, the record for
    # image 56 meets a window that is not full and is dropped at image 57 in favour of the SECOND one
    stamps_img = [im[0] for im in s["images"]]
    poses = np.loadtxt(jp)[:, 0]
    runs = [poses[0]] + [poses[k + 1] for k in np.flatnonzero(np.diff(poses) > 1.5 * synth.KF_DT)]
    assert np.allclose(runs, [stamps_img[10], stamps_img[32], stamps_img[57]], atol=1e-9), runs
    lv = host.last_vi_align()
    assert lv["stamps"][-1] == stamps_img[57] and lv["stamps"][0] == stamps_img[47] and len(lv["stamps"]) == 11
    # a stale record in front (stamped before the recording starts) is skipped, not applied to a later window
    stale = str(tmp_path / "stale.lfvt")
    wtr = trace.TraceWriter(stale)
    r0 = recs[0]
    wtr.sfm(r0["stamps"][0] - 5.0, r0["stamps"] - 5.0, r0["R"], r0["T"])
    for kind, payload in raw_records(dst):
        wtr._rec(kind, payload)
    wtr.close()
    c0 = fresh(host)
    rc, st2 = host.replay(stale, str(tmp_path / "traj2.txt"))
    assert rc == 0 and st2 == st and since(host, c0) == (3, 3)
    assert np.array_equal(np.loadtxt(jp), np.loadtxt(str(tmp_path / "traj2.txt")))
    assert ate.ate(jp, src)["n"] == st["poses"]


@pytest.mark.gpu
def test_records_that_are_not_applied(host, tmp_path):
    """A result that misses one frame's stamp is not passed to the device; one that fails LinearAlignment's gate (T mirrored: s < 0,
    status 1) is; either way the estimator stays initializing, the window slides, and the next valid record is taken."""
    from lfvio.engine import Engine  # noqa: F401

    src = str(tmp_path / "boot.lfvt")
    s = trace.make_stream(src, seed=3, n_frames=40)
    stamps = [t for t, *_ in s["truth"]]
    for kind, want_calls in (("missing", (1, 1)), ("gate", (2, 1))):
        dst = str(tmp_path / f"{kind}.lfvt")
        wtr = trace.TraceWriter(dst)
        n_img = 0
        for k, payload in raw_records(src):
            if k == trace.REC_BOOTSTRAP:
                continue
            if k == trace.REC_FEATURES:
                if n_img in (10, 11):  # in front of the first and the second full-window image
                    st_, R, T = truth_sfm(s, stamps[:n_img + 1], keyframe=2, scale=1.5)
                    if n_img == 10 and kind == "missing":
                        st_, R, T = np.delete(st_, 5), np.delete(R, 5, axis=0), np.delete(T, 5, axis=0)
                    if n_img == 10 and kind == "gate":
                        T = -T
                    wtr.sfm(stamps[n_img], st_, R, T)
                n_img += 1
            wtr._rec(k, payload)
        wtr.close()
        c0 = fresh(host)
        rc, st = host.replay(dst, str(tmp_path / f"{kind}.txt"))
        assert rc == 0 and st["last_status"] == 0 and st["bootstraps"] == 0, (kind, st)
        assert since(host, c0) == want_calls, (kind, since(host, c0))
        assert st["poses"] == st["images"] - 11, (kind, st)  # the first full window slid, the second aligned


@pytest.mark.gpu
def test_result_that_misses_a_non_keyframe(host, tmp_path):
    """40 px keyframe threshold: the image-frame list holds frames that are no keyframes of the window.  A result without ONE of
    those is not applied — no device call, the estimator keeps initializing and sliding — on two images in a row (initialization is
    attempted on at least one of them); the complete result that follows is taken."""
    from lfvio.engine import Engine  # noqa: F401

    p = str(tmp_path / "s3.lfvt")
    s = trace.make_stream(p, seed=3, n_frames=30)
    rd = trace.read_trace(p)
    c0 = fill_window(host, s, rd, n_images=14, px=40.0)
    host.set_stop_after_align(True)
    try:
        for n in range(14, 22):
            stamps = list(host.image_frames()[0]) + [s["images"][n][0]]
            kf = set(host.buffers()["stamps"][:W]) | {stamps[-1]}
            non_kf = [t for t in stamps if t not in kf]
            assert non_kf, "no non-keyframe in the list"
            st_, R, T = truth_sfm(s, stamps, keyframe=3, scale=2.5)
            if n < 16:  # incomplete: the first non-keyframe of the list is missing
                k = stamps.index(non_kf[0])
                st_, R, T = np.delete(st_, k), np.delete(R, k, axis=0), np.delete(T, k, axis=0)
            host.set_sfm(st_, R, T)
            fill_window(host, s, rd, n_images=n + 1, px=40.0, first=n)
            if n < 16:
                assert since(host, c0) == (0, 0) and host.flow()["solver_flag"] == 0 and host.flow()["frame_count"] == W
                assert not host.last_vi_align()["called"]
            elif since(host, c0) != (0, 0):
                break
    finally:
        host.set_stop_after_align(False)
    assert since(host, c0) == (1, 1) and n >= 16

