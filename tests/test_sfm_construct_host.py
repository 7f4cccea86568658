"""GlobalSFM::construct() on the host: relative pose records (trace type 9), WindowEstimator::constructSfm over lfvio_sfm_construct and
lfvio_sfm_ba, and the PnP loop and alignment behind it.

CPU: the record type round-trips through TraceWriter / read_trace; sfm_f as the host packs it equals a Python re-gather from the
recording (tests/flow_ref.py's feature list: every track in list order, frames start_frame ..., the bearings as stored) — without a
device the attempt then reports LFVIO_ERR_DEVICE and the window slides MARGIN_OLD.

GPU: on a short synthetic recording whose relative pose is computed from ground truth the way relativePose() intends it (the rotation
and unit-norm position of the newest camera in frame l): the captured inputs equal the re-gather bit for bit; the SfmStructure the host
filled equals Engine.sfm_construct + Engine.sfm_ba on those inputs bit for bit; the same images with that structure handed over as an
SfM structure leave a bit-identical aligned window; a record that makes the chain fail (a NaN translation: the first PnP is not finite,
status 2) slides MARGIN_OLD and a later image initializes; a recording with the two topics and one relative pose record replays to the end.
"""
import os
import sys

import numpy as np
import pytest

import flow_ref
import sfm_chain_ref as cr
from lfvio import abi, synth, trace
from test_pnp_host import fill_window, fresh, image_arrays, raw_records, since, steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = abi.WINDOW_SIZE
L_REF = 3  # the l of the records made here


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as ge

    ge.build()
    from lfvio.host import HostEstimator

    h = HostEstimator()
    yield h
    h.close()


def rename_returning_ids(images):
    """trace.make_stream lets a feature leave the 40 - 120 degree annulus and come back under its id.  A tracker never does that, and
    sfm_f counts a track's frames on from start_frame (estimator.cpp:257-263): such a track is triangulated from the wrong frames, far
    off, and the least-squares PnP behind it is lost.  Here an id that was not seen in the image before gets a new one (from 10^6)."""
    last, cur, nxt, out = {}, {}, 10 ** 6, []
    for k, (stamp, ids, xyz, uv, vel) in enumerate(images):
        ids = ids.copy()
        for j, i in enumerate(ids):
            i = int(i)
            if i in last and last[i] != k - 1:
                cur[i], nxt = nxt, nxt + 1
            last[i] = k
            ids[j] = cur.get(i, i)
        out.append((stamp, ids, xyz, uv, vel))
    return out


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """30 images of trace.make_stream at 0.1 px, returning ids renamed, as a file and in memory.  (At the default 1 px the chain completes
    but EPnP on bearings through z = 0 starts the bundle adjustment at a cost of 500 - 1 400, 50 iterations do not converge and the noise
    floor of the cost, 0.03, is above :283's 5e-3: the attempt is not accepted, here and with these arithmetic steps in the reference.)"""
    d = tmp_path_factory.mktemp("construct")
    src, p = str(d / "src.lfvt"), str(d / "s3.lfvt")
    s = trace.make_stream(src, seed=3, n_frames=30, pixel_noise=0.1)
    s["images"] = rename_returning_ids(s["images"])
    w, k = trace.TraceWriter(p), 0
    for kind, payload in raw_records(src):
        if kind == trace.REC_FEATURES:
            a = np.frombuffer(payload[12:], dtype="<f4").reshape(-1, 9).copy()
            a[:, 3] = s["images"][k][1]
            payload, k = payload[:12] + a.tobytes(), k + 1
        w._rec(kind, payload)
    w.close()
    return p, s, trace.read_trace(p)


def truth_relative(s, kf, l=L_REF):
    by = {t: (P, R) for t, P, R, _ in s["truth"]}
    return trace.relative_pose_from_truth([by[t][0] for t in kf], [by[t][1] for t in kf], l)


def sfm_f_of(ref):
    """estimator.cpp:255-269 on flow_ref's feature list -> (ids, offset, frame, bearing)."""
    ids, off, frm, us = [], [0], [], []
    for fid, start, obs in ref.feature:
        ids.append(fid)
        frm += list(range(start, start + len(obs)))
        us += obs
        off.append(len(frm))
    return np.array(ids, np.int32), np.array(off, np.int32), np.array(frm, np.int32), np.array(us)


def attempt(host, s, rd, px, record, first=14, last=22, stop=True):
    """A full window, then images with record(kf stamps) -> (R, T) or None handed over before each, until an attempt reaches constructSfm().
    flow_ref runs beside the host.  -> dict(n, kf, gather (sfm_f at the attempt), before (the state), c0, k0, flow (before the image))."""
    c0, _ = fill_window(host, s, rd, first, px=px)
    k0 = host.construct_counts()
    ref = flow_ref.Flow(px / 160.0)
    host.set_stop_after_align(stop)
    try:
        for stamp, idx, calls in steps(s, rd):
            if idx >= last:
                break
            for dt, a, g in calls:
                ref.process_imu(dt, a, g)
            _, ids, pts = image_arrays(s["images"][idx])
            if idx < first:
                ref.process_image(ids, pts, stamp)
                continue
            kf = list(host.buffers()["stamps"][:W]) + [stamp]
            assert np.array_equal(ref.Headers[:W], kf[:W])
            before, flow = host.state(), host.flow()
            rel = record(kf)
            if rel is not None:
                host.set_relative_pose(L_REF, *rel)
            for dt, a, g in calls:
                host.process_imu(dt, a, g)
            rc = host.process_image(stamp, ids, pts)
            ref.marg_old = ref.add_feature_check_parallax(ref.frame_count, ids, pts)
            ref.Headers[W] = stamp
            if host.last_construct()["calls"] != k0[0] or rc == -2:  # (-2: LFVIO_ERR_DEVICE, the attempt of a host without a device)
                return dict(n=idx, kf=kf, gather=sfm_f_of(ref), before=before, c0=c0, k0=k0, flow=flow, rc=rc, parallax_old=ref.marg_old)
            ref.slide_window()
    finally:
        host.set_stop_after_align(False)
    raise AssertionError("no attempt reached constructSfm()")


def same_inputs(lc, gather, rel):
    return (all(np.array_equal(a, b) for a, b in zip((lc["ids"], lc["offset"], lc["frame"], lc["bearing"]), gather)) and lc["F"] == W + 1 and lc["l"] == L_REF
            and np.array_equal(lc["relative_R"], rel[0]) and np.array_equal(lc["relative_T"], rel[1]))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_relative_pose_records_round_trip(tmp_path):
    p = str(tmp_path / "r.lfvt")
    w = trace.TraceWriter(p)
    R, T = synth.exp_so3(np.array([0.1, -0.2, 0.3])), np.array([0.6, 0.0, -0.8])
    w.imu(0.0, (0, 0, 9.8), (0, 0, 0))
    w.relative_pose(1.25, 4, R, T)
    w.structure(1.25, [1.0], [[1, 0, 0, 0]], [[0, 0, 0]], [7], [[1, 2, 3]])
    w.close()
    rd = trace.read_trace(p)
    assert rd["order"] == [trace.REC_IMU, trace.REC_RELATIVE, trace.REC_STRUCTURE] and len(rd["relatives"]) == 1 and len(rd["structures"]) == 1
    r = rd["relatives"][0]
    assert r["stamp"] == 1.25 and r["l"] == 4 and np.array_equal(r["R"], R) and np.array_equal(r["T"], T) and r["at_image"] == 0
    R2, T2 = trace.relative_pose_from_truth([[0, 0, 0], [1, 0, 0], [3, 0, 0]], [np.eye(3)] * 3, 1, tic=np.zeros(3), ric=np.eye(3))
    assert np.array_equal(R2, np.eye(3)) and np.array_equal(T2, [1, 0, 0])


def test_packing_and_err_device_without_a_gpu(host, stream):
    """Without a device: sfm_f as packed equals the re-gather, the attempt reports LFVIO_ERR_DEVICE before any call, the estimator keeps
    initializing and the slide is MARGIN_OLD (estimator.cpp:284).  (With a device the GPU tests cover the same packing.)"""
    import torch

    if torch.cuda.is_available():
        return
    p, s, rd = stream
    for px in (10.0, 40.0):
        a = attempt(host, s, rd, px, lambda kf: truth_relative(s, kf))
        lc = host.last_construct()
        assert a["rc"] == -2 and lc["rc"] == -2 and not lc["called"] and not lc["ba_called"] and lc["calls"] == a["k0"][0]
        assert same_inputs(lc, a["gather"], truth_relative(s, a["kf"])), px
        f = host.flow()
        assert f["solver_flag"] == 0 and f["marginalization_flag"] == abi.MARGIN_OLD and f["sum_of_back"] == a["flow"]["sum_of_back"] + 1
        assert host.construct_counts() == a["k0"] and since(host, a["c0"]) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("px", [10.0, 40.0])
def test_inputs_structure_and_the_structure_twin(host, stream, px):
    """stop_after_align on the first attempt: (1) last_construct's inputs equal the re-gather bit for bit; (2) what the host kept of the
    two device calls, and the SfmStructure it filled, equal Engine.sfm_construct + Engine.sfm_ba on those inputs bit for bit (:295-314: Q,
    T of the bundle adjustment, the ids and positions of the triangulated points); the structure is the truth's up to the noise (0.1 px:
    rotation matrices within 0.01, camera positions within 0.02 of the unit baseline); (3) the same images with that structure handed over through
    set_sfm_structure leave a bit-identical aligned window state and gravity."""
    from lfvio.engine import Engine

    p, s, rd = stream
    a = attempt(host, s, rd, px, lambda kf: truth_relative(s, kf))
    rel = truth_relative(s, a["kf"])
    lc = host.last_construct()
    assert lc["called"] and lc["ba_called"] and lc["rc"] == 0 and lc["ba_rc"] == 0 and lc["calls"] == a["k0"][0] + 1
    assert host.construct_counts() == (a["k0"][0] + 1, a["k0"][1] + 1) and since(host, a["c0"]) == (1, 1) and host.flow()["solver_flag"] == 0
    assert same_inputs(lc, a["gather"], rel)  # (1)
    eng = Engine(0)
    try:
        d = eng.sfm_construct(lc["F"], lc["l"], lc["offset"], lc["frame"], lc["bearing"], rel[0], rel[1])
        for k in ("c_rotation", "c_translation", "position", "tri_op"):
            assert d[k].tobytes() == lc[k].tobytes(), k
        assert d["status"] == 0 and lc["out"]["status"] == 0 and np.array_equal(d["pnp_count"], lc["out"]["pnp_count"]) and d["num_triangulated"] == lc["out"]["num_triangulated"]
        cp = cr.compact(d, lc["offset"], lc["frame"], lc["bearing"])
        b = eng.sfm_ba(lc["l"], cp["off"], cp["frame"], cp["bearing"], d["c_rotation"], d["c_translation"], cp["position"])
    finally:
        eng.close()
    st = host.sfm_structure()
    assert b["accepted"] == 1 and lc["ba"]["accepted"] == 1 and b["final_cost"] == lc["ba"]["final_cost"]
    assert np.array_equal(st["stamps"], a["kf"]) and st["Q"].tobytes() == b["Q"].tobytes() and st["T"].tobytes() == b["T"].tobytes()  # (2)
    assert np.array_equal(st["ids"], lc["ids"][cp["keep"]]) and st["xyz"].tobytes() == b["position"].tobytes()
    by = {t: (P, R) for t, P, R, _ in s["truth"]}
    Ps, Rs = np.array([by[t][0] for t in a["kf"]]), np.array([by[t][1] for t in a["kf"]])
    base = np.linalg.norm((Ps[-1] + Rs[-1] @ synth.TIC) - (Ps[L_REF] + Rs[L_REF] @ synth.TIC))
    tr = trace.structure_from_truth(a["kf"], Ps, Rs, [], np.zeros((0, 3)), keyframe=L_REF, scale=base)
    dR = max(np.abs(synth.q_to_R(st["Q"][k]) - synth.q_to_R(tr[1][k])).max() for k in range(W + 1))
    dT = np.abs(st["T"] - tr[2]).max()
    print(f"px {px}: image {a['n']}, {len(lc['ids'])} tracks, {lc['out']['num_triangulated']} triangulated, PnP counts {lc['out']['pnp_count'].tolist()}, "
          f"BA {lc['ba']['num_iterations']} iterations, final cost {lc['ba']['final_cost']:.3e}; to the truth: R {dR:.2e}, T {dT:.2e} (unit baseline)")
    assert dR < 0.01 and dT < 0.02
    got = host.state()
    got["g"], kf_stamps, lv = host.gravity(), host.buffers()["stamps"].copy(), host.last_vi_align()
    # (3) the structure twin
    c0, _ = fill_window(host, s, rd, a["n"], px=px)
    host.set_stop_after_align(True)
    try:
        host.set_sfm_structure(st["stamps"], st["Q"], st["T"], st["ids"], st["xyz"])
        fill_window(host, s, rd, a["n"] + 1, px=px, first=a["n"])
    finally:
        host.set_stop_after_align(False)
    assert since(host, c0) == (1, 1) and host.construct_counts() == (a["k0"][0] + 1, a["k0"][1] + 1) and np.array_equal(host.buffers()["stamps"], kf_stamps)
    other = host.state()
    other["g"] = host.gravity()
    lv2 = host.last_vi_align()
    assert lv["R"].tobytes() == lv2["R"].tobytes() and lv["T"].tobytes() == lv2["T"].tobytes()
    for k in ("Ps", "Rs", "Vs", "Bas", "Bgs", "g"):
        assert got[k].tobytes() == other[k].tobytes(), k


@pytest.mark.gpu
def test_a_failed_chain_slides_margin_old_and_a_later_image_initializes(host, stream):
    """A record with a NaN translation: every triangulated point is NaN, the first PnP (frame l + 1) trips its finiteness gate, the chain
    stops with status 2; no bundle adjustment, no PnP loop, no alignment; the estimator keeps initializing and the slide is MARGIN_OLD
    (estimator.cpp:284) whatever the parallax test said.  With true records from then on a later image initializes."""
    from lfvio.engine import Engine  # noqa: F401  (torch first: the ROCm wheel brings its own HIP runtime)

    p, s, rd = stream
    px = 40.0
    pnp0 = host.last_pnp()["calls"]
    a = attempt(host, s, rd, px, lambda kf: (truth_relative(s, kf)[0], np.full(3, np.nan)), stop=False)
    lc, f = host.last_construct(), host.flow()
    assert lc["called"] and lc["rc"] == 0 and lc["out"]["status"] == 2 and lc["out"]["failed_frame"] == L_REF + 1 and not lc["ba_called"]
    assert host.construct_counts() == (a["k0"][0] + 1, a["k0"][1]) and since(host, a["c0"]) == (0, 0) and host.last_pnp()["calls"] == pnp0
    assert f["solver_flag"] == 0 and f["frame_count"] == W and f["marginalization_flag"] == abi.MARGIN_OLD and f["sum_of_back"] == a["flow"]["sum_of_back"] + 1
    host.set_stop_after_align(True)
    try:
        for n in range(a["n"] + 1, a["n"] + 6):
            kf = list(host.buffers()["stamps"][:W]) + [s["images"][n][0]]
            host.set_relative_pose(L_REF, *truth_relative(s, kf))
            fill_window(host, s, rd, n + 1, px=px, first=n)
            if since(host, a["c0"]) != (0, 0):
                break
    finally:
        host.set_stop_after_align(False)
    assert since(host, a["c0"]) == (1, 1) and host.construct_counts() == (a["k0"][0] + 2, a["k0"][1] + 1) and n > a["n"]
    print(f"failed at image {a['n']} (parallax test said {'MARGIN_OLD' if a['parallax_old'] else 'MARGIN_SECOND_NEW'}), initialized at image {n}; "
          f"{len(host.last_pnp()['stamps'])} non-keyframes posed")


@pytest.mark.gpu
def test_a_recording_with_one_relative_pose_record_replays_to_the_end(host, stream, tmp_path):
    """The two topics and ONE relative pose record (no bootstrap, no SfM record): one construct, one alignment, a pose per image from then on."""
    from lfvio.engine import Engine  # noqa: F401

    p, s, rd = stream
    a = attempt(host, s, rd, 10.0, lambda kf: truth_relative(s, kf))
    dst, jp = str(tmp_path / "rel.lfvt"), str(tmp_path / "traj.txt")
    w = trace.TraceWriter(dst)
    for kind, payload in raw_records(p):
        if kind == trace.REC_BOOTSTRAP:
            continue
        if kind == trace.REC_FEATURES and np.frombuffer(payload[:8], "<f8")[0] == a["kf"][-1]:
            w.relative_pose(a["kf"][-1], L_REF, *truth_relative(s, a["kf"]))
        w._rec(kind, payload)
    w.close()
    tr = trace.read_trace(dst)
    assert len(tr["relatives"]) == 1 and tr["relatives"][0]["at_image"] == a["n"] and not tr["bootstraps"] and not tr["sfms"] and not tr["structures"]
    c0, k0 = fresh(host), host.construct_counts()
    rc, st = host.replay(dst, jp)
    assert rc == 0 and st["last_status"] == 0 and st["failures"] == 0 and st["bootstraps"] == 0, st
    assert since(host, c0) == (1, 1) and host.construct_counts() == (k0[0] + 1, k0[1] + 1) and host.flow()["solver_flag"] == 1
    assert st["poses"] == sum(im[0] >= a["kf"][-1] for im in s["images"][:st["images"]]) > 10, st
