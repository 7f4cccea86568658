"""The PnP loop of initialStructure() on the host: ImageFrame::points, SfM structure records (trace type 8),
WindowEstimator::solvePnpFrames over lfvio_pnp, and the alignment behind it.

CPU: the record type round-trips through TraceWriter / read_trace / Trace::load and a recording with types 3 and 7 reads as
before; over the oracle-backed C-ABI (which has no lfvio_pnp) the route reports LFVIO_ERR_DEVICE; the image-frame list keeps and
erases `points` in step with its entries across both kinds of slide and a reset.

GPU: the host's non-keyframe poses against the numpy restatement (tests/pnp_ref.py + estimator.cpp:353-356) on the host's own
inputs, and the aligned window state against the one reached by pushing the restated poses through set_sfm; recordings with
structure records replayed to the end (one at a 40 px keyframe threshold, so that the PnP loop has frames to pose; one with
reboots); structures that are not applied.

Measured values and bars are in the docstrings of the tests.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import flow_ref
import pnp_ref as pr
import vialign_ref as va
from lfvio import abi, synth, trace
from test_pnp import EPS, METRICS, loose_bar

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


def steps(s, rd):
    return flow_ref.sync(rd["imu"], [(im[0], None) for im in s["images"]], lambda: synth.TD0)


def fill_window(host, s, rd, n_images, px=10.0, first=0):
    """Feed images [first, n_images) without any record (first = 0: from a cleared estimator) -> the status of the last image."""
    c0 = fresh(host, px) if first == 0 else None
    rc = 0
    for stamp, idx, calls in steps(s, rd):
        if idx >= n_images:
            break
        if idx < first:
            continue
        for dt, a, g in calls:
            host.process_imu(dt, a, g)
        _, ids, pts = image_arrays(s["images"][idx])
        rc = host.process_image(stamp, ids, pts)
    return c0, rc


def truth_structure(s, kf_stamps, **kw):
    """The structure of the window whose keyframes carry kf_stamps, from the recording's truth: every landmark seen in them."""
    by = {t: (P, R) for t, P, R, _ in s["truth"]}
    img = {im[0]: im for im in s["images"]}
    seen = sorted({int(i) for t in kf_stamps for i in img[t][1]})
    return trace.structure_from_truth(kf_stamps, [by[t][0] for t in kf_stamps], [by[t][1] for t in kf_stamps], seen,
                                      s["Xw"][[s["id_point"][i] for i in seen]], **kw)


def restated_sfm(lp, st, list_stamps):
    """estimator.cpp:288-357 restated on the host's own PnP inputs: (R [F, 3, 3], T [F, 3]) over the image-frame list."""
    stamps, Q, T = st[0], st[1], st[2]
    R_out, T_out = np.zeros((len(list_stamps), 3, 3)), np.zeros((len(list_stamps), 3))
    res = pr.pnp(lp["offset"], lp["pw"], lp["us"]) if len(lp["stamps"]) else []
    for k, t in enumerate(list_stamps):
        j = np.flatnonzero(np.asarray(stamps) == t)
        if len(j):
            R_out[k], T_out[k] = synth.q_to_R(Q[j[0]]) @ synth.RIC.T, T[j[0]]
        else:
            q = int(np.flatnonzero(lp["stamps"] == t)[0])
            assert res[q]["status"] == 0
            R_out[k], T_out[k] = pr.post_process(res[q]["R"], res[q]["T"], synth.RIC)
    return R_out, T_out, res


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_structure_records_round_trip(host, tmp_path):
    """TraceWriter.structure -> read_trace and Trace::load give the record back; a recording with types 3 and 7 reads as before."""
    src, dst, sfm = str(tmp_path / "boot.lfvt"), str(tmp_path / "st.lfvt"), str(tmp_path / "sfm.lfvt")
    s = trace.make_stream(src, seed=7, n_frames=24)
    recs = trace.bootstraps_to_structure(src, dst, s, keyframe=2, scale=3.0)
    trace.bootstraps_to_sfm(src, sfm, keyframe=2, scale=3.0)
    a, b, c = trace.read_trace(src), trace.read_trace(dst), trace.read_trace(sfm)
    assert a["structures"] == [] and c["structures"] == [] and len(a["bootstraps"]) == 1 and len(c["sfms"]) == 2 and len(b["bootstraps"]) == 0 and b["sfms"] == []
    assert [k for k in a["order"] if k != trace.REC_BOOTSTRAP] == [k for k in b["order"] if k != trace.REC_STRUCTURE]
    assert np.array_equal(a["imu"], b["imu"]) and np.array_equal(a["truth"], b["truth"]) and len(a["images"]) == len(b["images"])
    assert len(b["structures"]) == 2
    r = b["structures"][0]
    assert r["at_image"] == 10 and r["stamp"] == b["images"][10][0] and np.array_equal(r["stamps"], [t for t, _ in b["images"][:11]])
    for k in ("stamps", "Q", "T", "ids", "xyz"):
        assert np.array_equal(r[k], recs[0][k]), k
    assert np.allclose(r["Q"][2], [1, 0, 0, 0], atol=1e-12) and np.allclose(r["T"][2], 0, atol=1e-12)  # the camera frame of keyframe 2
    # a landmark of the structure, seen from keyframe 5, lies along its bearing there
    img5 = s["images"][5]
    i = int(img5[1][0])
    X = r["xyz"][list(r["ids"]).index(i)]
    xc = synth.q_to_R(r["Q"][5]).T @ (X - r["T"][5])
    assert np.linalg.norm(xc / np.linalg.norm(xc) - img5[2][0] / np.linalg.norm(img5[2][0])) < 0.05
    # the same through the C++ loader
    L = host.L
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.lfvio_host_trace_structures.argtypes = [C.c_char_p, C.c_int, dp, ip, dp, C.c_int, dp, C.c_int]
    st, cnt = np.zeros(4), np.zeros((4, 2), dtype=np.int32)
    kf, pts = np.zeros((11, 8)), np.zeros((len(r["ids"]), 4))
    n = L.lfvio_host_trace_structures(dst.encode(), 4, st.ctypes.data_as(dp), cnt.ctypes.data_as(ip), kf.ctypes.data_as(dp), 11, pts.ctypes.data_as(dp), len(pts))
    assert n == 2 and st[0] == r["stamp"] and list(cnt[0]) == [11, len(r["ids"])]
    assert np.array_equal(kf[:, 0], r["stamps"]) and np.array_equal(kf[:, 1:5], r["Q"]) and np.array_equal(kf[:, 5:], r["T"])
    assert np.array_equal(pts[:, 0], r["ids"]) and np.array_equal(pts[:, 1:], r["xyz"])
    for other in (src, sfm):
        assert L.lfvio_host_trace_structures(other.encode(), 4, st.ctypes.data_as(dp), cnt.ctypes.data_as(ip), None, 0, None, 0) == 0
    L.lfvio_host_trace_sfms.argtypes = [C.c_char_p, C.c_int, dp, ip, dp, dp, C.c_int]
    fr = np.zeros(4, dtype=np.int32)
    assert L.lfvio_host_trace_sfms(sfm.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), None, None, 0) == 2 and fr[0] == 11
    assert L.lfvio_host_trace_sfms(dst.encode(), 4, st.ctypes.data_as(dp), fr.ctypes.data_as(ip), None, None, 0) == 0
    # a record whose length does not match its counts is refused like any malformed record
    raw = open(dst, "rb").read()
    bad = str(tmp_path / "bad.lfvt")
    open(bad, "wb").write(raw[:8] + (8).to_bytes(4, "little") + (24).to_bytes(4, "little") + b"\0" * 8 + (3).to_bytes(4, "little") + (1).to_bytes(4, "little") + b"\0" * 8)
    assert L.lfvio_host_trace_structures(bad.encode(), 4, st.ctypes.data_as(dp), cnt.ctypes.data_as(ip), None, 0, None, 0) == -1


def structure_before_image(host, s, n, **kw):
    """Hand over the structure of the window as image n will find it -> (the image-frame list's stamps then, the structure)."""
    stamps = list(host.image_frames()[0]) + [s["images"][n][0]]
    kf = list(host.buffers()["stamps"][:W]) + [stamps[-1]]
    st = truth_structure(s, kf, **kw)
    host.set_sfm_structure(*st)
    return stamps, kf, st


def test_oracle_abi_reports_err_device(oracle, tmp_path):
    """The CPU checker's C-ABI has no lfvio_pnp: with a non-keyframe in the list (40 px) the structure route reports
    LFVIO_ERR_DEVICE before any device call, the estimator is still initializing and its window slides."""
    from oracle import binding as ob

    from lfvio.host import HostEstimator

    p = str(tmp_path / "s3.lfvt")
    s = trace.make_stream(p, seed=3, n_frames=30)
    rd = trace.read_trace(p)
    h = HostEstimator(ob.build_host_oracle())
    fill_window(h, s, rd, 14, px=40.0)
    seen = False
    for n in range(14, 18):
        stamps, kf, _ = structure_before_image(h, s, n, keyframe=3, scale=2.5)
        _, rc = fill_window(h, s, rd, n + 1, px=40.0, first=n)
        lp = h.last_pnp()
        if lp["rc"] == -2:  # (initialization is attempted on every other image)
            assert rc == -2 and not lp["called"] and lp["calls"] == 0 and len(lp["stamps"]) == len(stamps) - len(kf) > 0
            seen = True
            break
    assert seen and h.flow()["solver_flag"] == 0 and h.flow()["frame_count"] == W and h.vi_align_counts() == (0, 0)
    h.close()


@pytest.mark.parametrize("px", [10.0, 40.0])
def test_image_frame_points_bookkeeping(host, tmp_path, px):
    """ImageFrame::points over 20 images without any initialization record: every entry of the list holds its image's feature ids
    in ascending order with their bearings, entries leave with a MARGIN_OLD slide (estimator.cpp:1051-1067) and stay with
    MARGIN_SECOND_NEW; reset() clears the list."""
    p = str(tmp_path / "s7.lfvt")
    s = trace.make_stream(p, seed=7, n_frames=24)
    rd = trace.read_trace(p)
    fresh(host, px)
    ref = flow_ref.Flow(px / 160.0)
    want, kinds = [], set()
    for stamp, idx, calls in steps(s, rd):
        if idx >= 20:
            break
        for dt, a, g in calls:
            host.process_imu(dt, a, g)
            ref.process_imu(dt, a, g)
        full, t0 = ref.frame_count == W, ref.Headers[0]
        _, ids, pts = image_arrays(s["images"][idx])
        perm = np.random.default_rng(idx).permutation(len(ids))  # (pushImage sorts: the order of arrival does not matter)
        assert host.process_image(stamp, ids[perm], pts[perm]) == 0
        ref.process_image(ids, pts, stamp)
        order = np.argsort(ids, kind="stable")
        want.append((stamp, ids[order], pts[order, :3]))
        if full and ref.marg_old:
            want = [e for e in want if e[0] > t0]
        if full:
            kinds.add(bool(ref.marg_old))
        st, _ = host.image_frames()
        assert list(st) == [e[0] for e in want], idx
        for k, (_, wi, wp) in enumerate(want):
            gi, gp = host.image_frame_points(k)
            assert np.array_equal(gi, wi) and np.array_equal(gp, wp), (idx, k)
        assert host.image_frame_points(len(want)) is None
    assert len(want) >= W and (px < 20 or (kinds == {True, False} and len(want) > W))
    host.clear_state()
    assert len(host.image_frames()[0]) == 0 and host.image_frame_points(0) is None


# ---------------------------------------------------------------------------------------------------------------- GPU
def align_on_structure(host, s, rd, px, **kw):
    """A full window, then structures until one aligns (stop_after_align) -> (list stamps, keyframe stamps, structure, state before)."""
    c0, _ = fill_window(host, s, rd, 14, px=px)
    host.set_stop_after_align(True)
    try:
        for n in range(14, 20):
            before = host.state()
            stamps, kf, st = structure_before_image(host, s, n, **kw)
            fill_window(host, s, rd, n + 1, px=px, first=n)
            if since(host, c0) != (0, 0):
                break
    finally:
        host.set_stop_after_align(False)
    assert since(host, c0) == (1, 1) and host.flow()["solver_flag"] == 0
    return n, stamps, kf, st, before


@pytest.mark.gpu
@pytest.mark.parametrize("px", [10.0, 40.0])
def test_host_poses_and_state_equal_the_restatement(host, tmp_path, px):
    """Test 7.  solvePnpFrames() + visualInitialAlign() on a full window, from a structure made of the truth (the camera frame of
    keyframe 3, scale 2.5, 0.1 deg / 0.5 % / 0.5 % noise on Q, T and the points).

    (a) On the host's own inputs (last_pnp) every non-keyframe's ImageFrame::R and T equal pnp_ref + estimator.cpp:353-356 within
    bar + REF of tests/test_pnp.py (R in eps, T in eps x the largest |x_w|); the keyframes' equal Q RIC^T and T of the structure to
    4 eps (one 3 x 3 product).
    (b) The aligned window state equals the one a second estimator reaches from the same images with the RESTATED poses pushed
    through set_sfm.  Bound, as in test_vi_align_host.py: 16 x the largest change of the restated state (vialign_ref) when every
    input moves by one ulp and, on top, every non-keyframe pose by its difference (a) at random signs, over three trials.  Without
    a non-keyframe in the list the two routes hand the alignment the same bits and the states are equal.
    Device figures: not measured."""
    from lfvio.engine import Engine  # noqa: F401  (torch first: the ROCm wheel brings its own HIP runtime)

    p = str(tmp_path / "s3.lfvt")
    s = trace.make_stream(p, seed=3, n_frames=30)
    rd = trace.read_trace(p)
    kw = dict(keyframe=3, scale=2.5, rot_noise_deg=0.1, pos_noise=0.005, point_noise=0.005, seed=11)
    n, stamps, kf, st, before = align_on_structure(host, s, rd, px, **kw)
    lp, lv = host.last_pnp(), host.last_vi_align()
    non_kf = [t for t in stamps if t not in set(kf)]
    assert px < 20 or non_kf, "no non-keyframe in the list"
    assert np.array_equal(lp["stamps"], non_kf) and lp["called"] == bool(non_kf) and lp["rc"] == 0
    assert np.array_equal(lv["stamps"], stamps) and lv["out"]["status"] == 0
    R_ref, T_ref, res = restated_sfm(lp, st, stamps)
    worst = dict(R=0.0, T=0.0)
    diff = np.zeros(len(stamps))
    for k, t in enumerate(stamps):
        dR, dT = np.abs(lv["R"][k] - R_ref[k]).max(), np.abs(lv["T"][k] - T_ref[k]).max()
        if t in set(kf):
            assert dR <= 4 * EPS and dT == 0.0, (k, dR, dT)
            continue
        q = int(np.flatnonzero(lp["stamps"] == t)[0])
        scale = float(np.abs(lp["pw"][lp["offset"][q]:lp["offset"][q + 1]]).max())
        worst["R"], worst["T"] = max(worst["R"], dR / EPS), max(worst["T"], dT / (EPS * scale))
        diff[k] = max(dR, dT)
        assert lp["out"][q]["status"] == 0 and lp["offset"][q + 1] - lp["offset"][q] >= 6
    print(f"px {px}: {len(non_kf)} non-keyframes of {len(stamps)} frames; host - restatement R {worst['R']:.3g} / bar {loose_bar('R'):.3g} eps, "
          f"T {worst['T']:.3g} / bar {loose_bar('T'):.3g} eps |x_w|")
    assert worst["R"] <= loose_bar("R") and worst["T"] <= loose_bar("T")
    got = host.state()
    got["g"] = host.gravity()
    kf_stamps = host.buffers()["stamps"]
    # the same images with the restated poses as an SfM result
    fill_window(host, s, rd, n, px=px)
    host.set_stop_after_align(True)
    try:
        host.set_sfm(stamps, R_ref, T_ref)
        fill_window(host, s, rd, n + 1, px=px, first=n)
    finally:
        host.set_stop_after_align(False)
    assert host.last_vi_align()["out"]["status"] == 0 and np.array_equal(host.buffers()["stamps"], kf_stamps)
    other = host.state()
    other["g"] = host.gravity()
    if not non_kf:
        for k in ("Ps", "Rs", "Vs", "Bgs", "g"):
            assert np.array_equal(got[k], other[k]), k
        return
    a = (lv["spans"], lv["noise"], lv["tic"], lv["G"])
    want = va.window_state_np(va.align_np(R_ref, T_ref, *a), R_ref, T_ref, stamps, kf_stamps, lv["tic"], before["Bgs"])
    change = {k: 0.0 for k in want}
    for trial in range(3):
        rng = np.random.default_rng(trial)
        pt = lambda v: np.nextafter(v, np.where(rng.random(np.shape(v)) < 0.5, -np.inf, np.inf))
        sg = lambda v: np.where(rng.random(np.shape(v)) < 0.5, -1.0, 1.0)
        R_, T_ = pt(R_ref) + sg(R_ref) * diff[:, None, None], pt(T_ref) + sg(T_ref) * diff[:, None]
        spans_ = [None] + [(sp[0], sp[1], pt(sp[2]), pt(sp[3]), sp[4], pt(sp[5]), pt(sp[6])) for sp in lv["spans"][1:]]
        w2 = va.window_state_np(va.align_np(R_, T_, spans_, *a[1:]), R_, T_, stamps, kf_stamps, lv["tic"], before["Bgs"])
        for k in want:
            change[k] = max(change[k], np.abs(w2[k] - want[k]).max())
    for k in want:
        d = np.abs(got[k] - other[k]).max()
        print(f"px {px} {k}: structure route - restated poses through set_sfm {d:.3g}, bar {16 * change[k]:.3g}")
        assert d <= 16 * change[k], k


def keyframes_by_flow(s, rd, px):
    """stamp of an image -> the stamps of the window's keyframes when that image arrives (the parallax test restated, flow_ref)."""
    ref, out = flow_ref.Flow(px / 160.0), {}
    for stamp, idx, calls in steps(s, rd):
        for dt, a, g in calls:
            ref.process_imu(dt, a, g)
        _, ids, pts = image_arrays(s["images"][idx])
        if ref.frame_count == W:
            out[stamp] = list(ref.Headers[:W]) + [stamp]
        ref.process_image(ids, pts, stamp)
    return lambda t: out[min(out, key=lambda u: abs(u - t))]


@pytest.mark.gpu
def test_structure_recording_replays_to_the_end(host, tmp_path):
    """Test 8a.  A 60-image recording at a 40 px keyframe threshold whose bootstrap record is replaced by structure records
    (noise-free, the camera frame of keyframe 4, everything divided by 2.5): no bootstrap, one PnP call with at least one frame,
    one alignment, a pose per image from the alignment on.  Its ATE against the ATE of the same recording fed a type-7 record made
    of pnp_ref's poses on the host's own PnP inputs: within 1 %, the agreement test_vi_align_host.py demands of its two routes.
    Device figures: not measured."""
    import ate
    from lfvio.engine import Engine  # noqa: F401

    src, dst, sfm = str(tmp_path / "boot.lfvt"), str(tmp_path / "st.lfvt"), str(tmp_path / "sfm.lfvt")
    s = trace.make_stream(src, seed=3, n_frames=60)
    rd = trace.read_trace(src)
    s["keyframes_of"] = keyframes_by_flow(s, rd, 40.0)
    recs = trace.bootstraps_to_structure(src, dst, s, keyframe=4, scale=2.5, repeat=6, skip=4)  # (images 14 .. 19: the list has non-keyframes by then)
    jp = {k: str(tmp_path / f"traj_{k}.txt") for k in ("st", "sfm")}
    c0 = fresh(host, 40.0)
    calls0 = host.last_pnp()["calls"]
    rc, st = host.replay(dst, jp["st"])
    assert rc == 0 and st["last_status"] == 0 and st["failures"] == 0 and st["bootstraps"] == 0, st
    lp, lv = host.last_pnp(), host.last_vi_align()
    assert since(host, c0) == (1, 1) and lp["calls"] - calls0 == 1 and lp["called"] and len(lp["stamps"]) >= 1
    assert st["poses"] == sum(im[0] >= lv["stamps"][-1] for im in s["images"][:st["images"]])
    # the type-7 twin: the restated poses of the same list
    tr_st = [r for r in trace.read_trace(dst)["structures"] if abs(r["stamp"] - lv["stamps"][-1]) < 1e-6][0]
    R_ref, T_ref, _ = restated_sfm(lp, (tr_st["stamps"], tr_st["Q"], tr_st["T"]), lv["stamps"])
    wtr = trace.TraceWriter(sfm)
    for kind, payload in raw_records(dst):
        if kind == trace.REC_STRUCTURE:
            continue
        if kind == trace.REC_FEATURES and abs(np.frombuffer(payload[:8], "<f8")[0] - lv["stamps"][-1]) < 1e-6:
            wtr.sfm(lv["stamps"][-1], lv["stamps"], R_ref, T_ref)
        wtr._rec(kind, payload)
    wtr.close()
    c0 = fresh(host, 40.0)
    rc, st2 = host.replay(sfm, jp["sfm"])
    assert rc == 0 and all(st2[k] == st[k] for k in ("images", "poses", "failures", "bootstraps", "keyframes", "non_keyframes")), (st, st2)
    assert since(host, c0) == (1, 1) and host.last_pnp()["calls"] == lp["calls"]
    e = {k: ate.ate(jp[k], src)["rmse"] for k in jp}
    print(f"ATE at 40 px: structure route {e['st']:.5f} m, pnp_ref's poses as a type-7 record {e['sfm']:.5f} m; "
          f"{len(lp['stamps'])} non-keyframes of {len(lv['stamps'])} frames, {lp['offset'][-1]} correspondences")
    assert abs(e["st"] / e["sfm"] - 1.0) < 0.01, e


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
def test_structure_reboots_mid_recording(host, tmp_path):
    """Test 8b.  test_flow's reboot recording (restart message before image 22, accelerometer spike before image 45) with
    structure records at the default threshold: one restart, one failure, three alignments, no bootstrap, the poses of the
    type-7 route of test_vi_align_host.py's twin test, which consumed the records of the same images."""
    from lfvio.engine import Engine  # noqa: F401

    src, dst = str(tmp_path / "boot.lfvt"), str(tmp_path / "st.lfvt")
    s = trace.make_stream(src, seed=9, n_frames=70, restart_at=22, spike_at=45)
    recs = trace.bootstraps_to_structure(src, dst, s, keyframe=1, scale=0.5)
    assert len(recs) == 3
    jp = str(tmp_path / "traj.txt")
    c0 = fresh(host)
    rc, st = host.replay(dst, jp)
    assert rc == 0 and st["last_status"] == 0, st
    assert st["restarts"] == 1 and st["failures"] == 1 and st["bootstraps"] == 0 and since(host, c0) == (3, 3), (st, since(host, c0))
    assert st["poses"] == st["images"] - 30 - 1, st
    stamps_img = [im[0] for im in s["images"]]
    poses = np.loadtxt(jp)[:, 0]
    runs = [poses[0]] + [poses[k + 1] for k in np.flatnonzero(np.diff(poses) > 1.5 * synth.KF_DT)]
    assert np.allclose(runs, [stamps_img[10], stamps_img[32], stamps_img[57]], atol=1e-9), runs


@pytest.mark.gpu
def test_structures_that_are_not_applied(host, tmp_path):
    """Test 9, at 40 px on two images in a row each (initialization is attempted on at least one of them): a structure that misses
    a keyframe of the window — no device call of either kind; a non-keyframe left with 5 correspondences — none either (the
    reference returns false at :335-340); both times the estimator keeps initializing and sliding.  Then a structure AND an SfM
    result for the same image: the SfM result wins, lfvio_pnp is not called, the alignment takes the result's poses."""
    from lfvio.engine import Engine  # noqa: F401

    p = str(tmp_path / "s3.lfvt")
    s = trace.make_stream(p, seed=3, n_frames=34)
    rd = trace.read_trace(p)
    c0, _ = fill_window(host, s, rd, 14, px=40.0)
    calls0 = host.last_pnp()["calls"]
    host.set_stop_after_align(True)
    try:
        for n in range(14, 24):
            stamps = list(host.image_frames()[0]) + [s["images"][n][0]]
            kf = list(host.buffers()["stamps"][:W]) + [stamps[-1]]
            non_kf = [t for t in stamps if t not in set(kf)]
            assert non_kf, "no non-keyframe in the list"
            st = truth_structure(s, kf, keyframe=3, scale=2.5)
            if n < 16:  # keyframe 5 is missing
                st = (np.delete(st[0], 5), np.delete(st[1], 5, axis=0), np.delete(st[2], 5, axis=0), st[3], st[4])
            elif n < 18:  # the first non-keyframe keeps 5 of its features in the structure
                ids_f = {int(i) for i in {im[0]: im for im in s["images"]}[non_kf[0]][1]}
                hit = [k for k, i in enumerate(st[3]) if int(i) in ids_f]
                assert len(hit) > 5
                st = (st[0], st[1], st[2], np.delete(st[3], hit[5:]), np.delete(st[4], hit[5:], axis=0))
            host.set_sfm_structure(*st)
            if n >= 18:
                by = {t: (P, R) for t, P, R, _ in s["truth"]}
                res = trace.sfm_from_truth(stamps, [by[t][0] for t in stamps], [by[t][1] for t in stamps], keyframe=3, scale=2.5)
                host.set_sfm(*res)
            fill_window(host, s, rd, n + 1, px=40.0, first=n)
            if n < 18:
                assert since(host, c0) == (0, 0) and host.flow()["solver_flag"] == 0 and host.flow()["frame_count"] == W, n
                lp = host.last_pnp()
                assert lp["calls"] == calls0 and not lp["called"], n
            elif since(host, c0) != (0, 0):
                break
    finally:
        host.set_stop_after_align(False)
    assert since(host, c0) == (1, 1) and n >= 18 and host.last_pnp()["calls"] == calls0
    lv = host.last_vi_align()
    assert np.array_equal(lv["R"], res[1]) and np.array_equal(lv["T"], res[2])
    # the structure handed over with that result was dropped with it: the next image does not find it
    assert host.flow()["solver_flag"] == 0
