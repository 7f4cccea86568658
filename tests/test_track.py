"""lfvio_track_reject / lfvio_track_undistort / lfvio_track_reset (k_trk_lift, k_tv_hyp, k_trk_fit, k_trk_undist) on the device, bit
for bit unless said, against tests/track_ref.py and against the device's own two-view path.

  1  the lift: bearing_cur / bearing_forw equal track_ref.bearings on every fixture case
  2  the RANSAC against lfvio_two_view on the restatement's bearings: status[], best_sample, num_inliers, best_score and E are equal —
     the same device functions on the same bits, so no tolerance and no case dropped; N over the edges of NR = max(N, 9), a wave,
     the fit's block and TV_CHUNK, S = 1, 100 and 1024
  3  the RANSAC against the restatement: status[] equals track_ref.reject's on the fixture cases; a case that breaks C1 / C2 on the
     restatement drops out, at most 10 % may (tests/test_track_ref.py asserts that none does)
  4  the status paths: 1 (pure noise: no hypothesis scores, or the winner keeps fewer than 8) and 2 (N = 0, 7)
  5  undistortedPoints: sequences against track_ref.Undistort
  6  argument errors, one per refused field of both calls
  7  repeatability, and both calls beside an optimization in flight"""
import ctypes as C
import os

import numpy as np
import pytest

import track_ref as tr

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "track_cases.npz"))
    return {k: z[k] for k in z.files}


def fixture_case(fx, name):
    return tr.cam_from_vector(fx[f"{name}/cam"]), fx[f"{name}/cur"], fx[f"{name}/forw"], fx[f"{name}/samples"]


def test_lift(eng, fx):
    """Test 1."""
    n = 0
    for name in tr.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if len(cur) < 8:
            continue
        d = eng.track_reject(cam, cur, forw, s, want_bearings=True)
        assert same(d["bearing_cur"], tr.bearings(cam, cur)) and same(d["bearing_forw"], tr.bearings(cam, forw)), name
        assert same(d["bearing_cur"], fx[f"{name}/bearing_cur"]) and same(d["bearing_forw"], fx[f"{name}/bearing_forw"]), name
        n += 1
    assert n >= 5
    # a spread of pixels over the whole image, both cameras (also outside the annulus: the polynomial is what it is there)
    rng = np.random.default_rng(8)
    px = rng.uniform([-50.0, -50.0], [1330.0, 1010.0], (2 * 1031, 2)).astype(np.float32)
    for cam in (tr.PAL, tr.SKEW):
        d = eng.track_reject(cam, px[:1031], px[1031:], tr.make_samples(1, 1031, 1), want_bearings=True)
        assert same(d["bearing_cur"], tr.bearings(cam, px[:1031])) and same(d["bearing_forw"], tr.bearings(cam, px[1031:]))


def against_two_view(eng, cam, cur, forw, s, tag):
    bl, br = tr.bearings(cam, cur), tr.bearings(cam, forw)
    t = eng.two_view(bl, br, s)
    d = eng.track_reject(cam, cur, forw, s)
    assert (d["status"], d["best_sample"], d["num_inliers"]) == (t["status"], t["best_sample"], t["num_inliers"]), tag
    assert np.float64(d["best_score"]).tobytes() == np.float64(t["best_score"]).tobytes(), tag
    if t["status"] == 0:
        assert same(d["mask"], t["mask"]) and same(d["E"], np.asarray(t["E"], np.float64).reshape(9)), tag
        assert int(d["mask"].sum()) == d["num_inliers"]
    else:
        assert np.all(d["mask"] == 1), tag
    return t["status"]


SIZES_N = (8, 9, 64, 65, 256, 257, 1024, 1025)


def test_ransac_equals_the_two_view_path(eng):
    """Test 2."""
    models = 0
    for i, N in enumerate(SIZES_N):
        cam = (tr.PAL, tr.SKEW)[i % 2]
        kw = dict(noise_px=0.2, outliers=0.0) if N < 30 else {}
        cur, forw = tr.make_matches(100 + i, cam, N, **kw)
        for S in (1, 100):
            models += against_two_view(eng, cam, cur, forw, tr.make_samples(200 + 2 * i + S, N, S), f"N={N} S={S}") == 0
    cur, forw = tr.make_matches(150, tr.PAL, 4096)
    models += against_two_view(eng, tr.PAL, cur, forw, tr.make_samples(151, 4096, 100), "N=4096 S=100") == 0
    cur, forw = tr.make_matches(152, tr.SKEW, 150)
    models += against_two_view(eng, tr.SKEW, cur, forw, tr.make_samples(153, 150, 1024), "N=150 S=1024") == 0
    assert models >= 9  # (S = 1 seldom finds a model: those cases compare the no-model record)


def test_ransac_equals_the_restatement(eng, fx):
    """Test 3."""
    dropped, total = [], 0
    for name in tr.CASES:
        cam, cur, forw, s = fixture_case(fx, name)
        if int(fx[f"{name}/status"]) != 0:
            continue
        total += 1
        r = tr.reject(cam, cur, forw, s)
        assert same(r["mask"], fx[f"{name}/mask"]), name
        if not tr.conditions(r):
            dropped.append(name)
            continue
        d = eng.track_reject(cam, cur, forw, s)
        assert d["status"] == 0 and d["best_sample"] == r["best_sample"] and d["num_inliers"] == r["num_inliers"], name
        assert same(d["mask"], r["mask"]), name
    assert total >= 4 and len(dropped) <= 0.1 * total, dropped


def no_model_cases():
    """Pure noise (N = 40, S = 1 .. 3: unrelated pixel clouds) on which the restatement reports (a) every hypothesis scoring
    exactly 0 and (b) a winner with a positive score and fewer than 8 inliers; up to two of each kind."""
    from golden import gen_twoview_hp as gen

    out = {"a": [], "b": []}
    for seed in range(400):
        rng = np.random.default_rng([seed, 78])
        cam = (tr.PAL, tr.SKEW)[seed % 2]
        cur = tr.project(cam, gen.annulus(rng, 40, (40.0, 120.0))).astype(np.float32)
        forw = tr.project(cam, gen.annulus(rng, 40, (40.0, 120.0))).astype(np.float32)
        s = tr.make_samples(seed, 40, 1 + seed % 3)
        r = tr.reject(cam, cur, forw, s)
        kind = "a" if r["best_sample"] < 0 else "b" if r["status"] == 1 else None
        if kind and len(out[kind]) < 2:
            out[kind].append((cam, cur, forw, s, r))
        if len(out["a"]) == 2 and len(out["b"]) == 2:
            break
    return out


def filled_out():
    from lfvio import abi

    out = abi.TrackRejectOutC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return out


def test_status_paths(eng):
    """Test 4."""
    cases = no_model_cases()
    assert cases["a"] or cases["b"]
    for kind in ("a", "b"):
        for cam, cur, forw, s, r in cases[kind]:
            assert r["status"] == 1 and np.all(r["mask"] == 1)  # the restatement, on the CPU
            out, mask = filled_out(), np.full(40, 5, np.uint8)
            d = eng.track_reject(cam, cur, forw, s, out=out, status=mask, want_bearings=True)
            assert d["rc"] == 0 and d["status"] == 1 and np.all(mask == 1)
            assert (d["best_sample"], d["num_inliers"]) == (r["best_sample"], r["num_inliers"]), kind
            assert bytes(out)[24:] == b"\x5a" * 72  # E untouched
            assert same(d["bearing_cur"], r["bearing_cur"]) and same(d["bearing_forw"], r["bearing_forw"])
            against_two_view(eng, cam, cur, forw, s, kind)
            if kind == "a":
                assert d["best_sample"] == -1 and d["num_inliers"] == 0 and d["best_score"] == 0.0
            else:
                assert d["best_sample"] >= 0 and 0 < d["num_inliers"] < 8 and d["best_score"] > 0
    cur, forw = tr.make_matches(7, tr.PAL, 7)
    for N in (0, 7):
        out, mask = filled_out(), np.full(8, 5, np.uint8)
        bc, bf = np.full((8, 3), 3.25), np.full((8, 3), 3.25)
        d = eng.track_reject(tr.PAL, cur[:N], forw[:N], None, out=out, status=mask, bearings=(bc, bf), num_samples=0)
        assert d["rc"] == 0 and (d["status"], d["best_sample"], d["num_inliers"], d["best_score"]) == (2, -1, 0, 0.0)
        assert np.all(mask[:N] == 1) and np.all(mask[N:] == 5) and bytes(out)[24:] == b"\x5a" * 72
        assert np.all(bc == 3.25) and np.all(bf == 3.25)
        assert tr.reject(tr.PAL, cur[:N], forw[:N], None)["status"] == 2


def run_sequence(eng, cam, calls):
    """calls: (pts, ids, time), or "reset".  Every call against the restatement's state object."""
    state = tr.Undistort()
    eng.track_reset()
    outs = []
    for k, call in enumerate(calls):
        if isinstance(call, str):
            state.reset()
            eng.track_reset()
            continue
        pts, ids, time = call
        r, d = state(cam, pts, ids, time), eng.track_undistort(cam, pts, ids, time)
        for key in ("un_pts", "un_pts_3d", "velocity_3d", "matched"):
            assert same(d[key], r[key]), (k, key)
        outs.append(r)
    return outs


def pixels(rng, cam, n):
    from golden import gen_twoview_hp as gen

    return tr.project(cam, gen.annulus(rng, n, (40.0, 120.0))).astype(np.float32)


def test_undistort_five_calls(eng):
    """Test 5, the ids: stay, vanish, come back, arrive as -1 and are numbered afterwards, several -1, a duplicate, a permuted
    order, dt = 0."""
    rng = np.random.default_rng(31)
    for cam in (tr.PAL, tr.SKEW):
        base = pixels(rng, cam, 12)
        move = lambda k: (base + np.float32(0.75 * k)).astype(np.float32)
        calls = [
            (move(0)[:8], [0, 1, 2, 3, 4, 5, -1, -1], 10.0),
            (move(1)[[7, 6, 5, 4, 2, 1, 0, 8, 9]], [7, 6, 5, 4, 2, 1, 0, -1, -1], 10.05),       # 3 vanishes; 6, 7: numbered afterwards
            (move(2)[[0, 1, 3, 6, 7, 8, 9, 4, 4]], [0, 1, 3, 6, 7, 8, 9, 4, 4], 10.1),           # 3 comes back, 4 twice
            (move(3)[[4, 0, 1, 3, 6, 10]], [4, 0, 1, 3, 6, -1], 10.1),                          # dt = 0
            (move(4)[[10, 6, 3, 1, 0, 4, 11]], [10, 6, 3, 1, 0, 4, -1], 10.15),
        ]
        outs = run_sequence(eng, cam, calls)
        assert not outs[0]["velocity_3d"].any()
        v1 = outs[1]["velocity_3d"]
        assert not v1[:2].any() and not v1[7:].any() and v1[2:7].any(axis=1).all()  # 7, 6 were -1 a call ago: zero on their second frame too
        assert list(outs[2]["matched"]) == [6, 5, -1, 1, 0, -1, -1, 3, 3]
        assert not np.isfinite(outs[3]["velocity_3d"][:5]).any() and not outs[3]["velocity_3d"][5].any()  # x / 0: inf or nan
        assert list(outs[4]["matched"]) == [-1, 4, 3, 2, 1, 0, -1]
    # the first occurrence of an id wins in the map
    p = pixels(rng, tr.PAL, 3)
    outs = run_sequence(eng, tr.PAL, [(p, [5, 5, 5], 1.0), (p[:1], [5], 2.0), (p[1:2], [5], 3.0)])
    assert outs[1]["matched"][0] == 0 and not outs[1]["velocity_3d"].any() and outs[2]["velocity_3d"].any()


def test_undistort_sizes_empty_map_and_reset(eng):
    """Test 5, the rest: N = 0 followed by a call whose velocities are all 0, lfvio_track_reset in the middle, N = 1, 63, 65 and 4096
    against a previous call of 1 and the other way round."""
    rng = np.random.default_rng(32)
    cam = tr.SKEW
    big = pixels(rng, cam, 4096)
    ids = rng.permutation(4096).astype(np.int32)
    t, calls = 5.0, []
    for n in (1, 63, 65, 4096):
        sel = rng.choice(4096, n, replace=False)
        one = int(sel[0]) if n < 4096 else 4095  # the id of the single point: among the n, for 4096 the last slot's
        j = int(np.flatnonzero(ids == ids[one])[0])
        calls += [(big[j:j + 1], ids[j:j + 1], t), (big[sel] + np.float32(0.5), ids[sel], t + 0.04),
                  (big[j:j + 1] + np.float32(1.0), ids[j:j + 1], t + 0.08)]
        t += 1.0
    calls.append((big, ids, t))
    calls.append((big[::-1] + np.float32(0.25), ids[::-1], t + 0.05))  # 4096 against 4096: the last index of the LDS table
    outs = run_sequence(eng, cam, calls)
    for k in range(4):
        assert (outs[3 * k + 1]["matched"] >= 0).sum() == 1 and outs[3 * k + 2]["matched"][0] >= 0, k
    assert same(outs[-1]["matched"], np.arange(4095, -1, -1, dtype=np.int32)) and outs[-1]["velocity_3d"].any(axis=1).all()
    p = pixels(rng, cam, 20)
    i20 = np.arange(20, dtype=np.int32)
    empty = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), 2.1)
    outs = run_sequence(eng, cam, [(p, i20, 2.0), empty, (p + np.float32(1), i20, 2.2), (p + np.float32(2), i20, 2.3), "reset", (p, i20, 2.4),
                                   (p + np.float32(1), i20, 2.5)])
    assert not outs[2]["velocity_3d"].any() and outs[3]["velocity_3d"].any(axis=1).all()
    assert not outs[4]["velocity_3d"].any() and outs[5]["velocity_3d"].any(axis=1).all()


def test_argument_errors(eng):
    """Test 6."""
    from lfvio import abi

    cam = tr.PAL
    cur, forw = tr.make_matches(61, cam, 40)
    s = tr.make_samples(62, 40, 5)
    hi, lo = s.copy(), s.copy()
    hi[2, 3], lo[0, 0] = 40, -1
    other = dict(cam, model=1)
    out, mask = filled_out(), np.full(40, 0x5A, np.uint8)
    bc, bf = np.full((40, 3), 3.25), np.full((40, 3), 3.25)
    kw = dict(out=out, status=mask, bearings=(bc, bf), check=False)
    refused = [
        eng.track_reject(None, cur, forw, s, **kw), eng.track_reject(other, cur, forw, s, **kw),
        eng.track_reject(cam, cur, forw, s, num_points=-1, **kw), eng.track_reject(cam, cur, forw, s, num_points=4097, **kw),
        eng.track_reject(cam, None, forw, s, num_points=40, **kw), eng.track_reject(cam, cur, None, s, **kw),
        eng.track_reject(cam, cur, forw, None, num_samples=5, **kw), eng.track_reject(cam, cur, forw, s, num_samples=0, **kw),
        eng.track_reject(cam, cur, forw, s, num_samples=1025, **kw), eng.track_reject(cam, cur, forw, hi, **kw),
        eng.track_reject(cam, cur, forw, lo, **kw),
        eng.track_reject(cam, None, None, None, num_points=3, num_samples=0, **kw),
    ]
    for k, d in enumerate(refused):
        assert d["rc"] == -1, k  # LFVIO_ERR_ARG
    ub = C.POINTER(C.c_ubyte)
    rin = abi.TrackRejectInC()
    assert eng.lib.lfvio_track_reject(eng.ctx, None, mask.ctypes.data_as(ub), C.byref(out), None, None) == -1
    assert eng.lib.lfvio_track_reject(eng.ctx, C.byref(rin), None, C.byref(out), None, None) == -1
    assert eng.lib.lfvio_track_reject(eng.ctx, C.byref(rin), mask.ctypes.data_as(ub), None, None, None) == -1
    assert eng.lib.lfvio_track_reject(None, C.byref(rin), mask.ctypes.data_as(ub), C.byref(out), None, None) == -1
    assert bytes(out) == b"\x5a" * C.sizeof(out) and np.all(mask == 0x5A) and np.all(bc == 3.25) and np.all(bf == 3.25)
    assert eng.track_reject(cam, cur, forw, s)["rc"] == 0

    # lfvio_track_undistort: outputs, the resident map and the time untouched
    rng = np.random.default_rng(63)
    p0, p1 = pixels(rng, cam, 30), pixels(rng, cam, 30)
    ids = np.arange(30, dtype=np.int32)
    eng.track_reset()
    eng.track_undistort(cam, p0, ids, 1.0)
    want = eng.track_undistort(cam, p1, ids, 1.25)
    assert want["velocity_3d"].any(axis=1).all()
    eng.track_reset()
    eng.track_undistort(cam, p0, ids, 1.0)
    outs = (np.full((30, 2), 7.5, np.float32), np.full((30, 3), 7.5, np.float32), np.full((30, 3), 7.5, np.float32), np.full(30, 77, np.int32))
    kw = dict(outs=outs, check=False)
    refused = [
        eng.track_undistort(None, p1, ids, 9.0, **kw), eng.track_undistort(other, p1, ids, 9.0, **kw),
        eng.track_undistort(cam, p1, ids, 9.0, num_points=-1, **kw), eng.track_undistort(cam, p1, ids, 9.0, num_points=4097, **kw),
        eng.track_undistort(cam, None, ids, 9.0, num_points=30, **kw), eng.track_undistort(cam, p1, None, 9.0, **kw),
        eng.track_undistort(cam, p1, ids, float("nan"), **kw),
    ]
    for k, d in enumerate(refused):
        assert d["rc"] == -1, k
    uin = abi.TrackUndistortInC()
    fp = C.POINTER(C.c_float)
    o = [a.ctypes.data_as(fp) for a in outs[:3]]
    assert eng.lib.lfvio_track_undistort(eng.ctx, None, o[0], o[1], o[2], None) == -1
    assert eng.lib.lfvio_track_undistort(None, C.byref(uin), o[0], o[1], o[2], None) == -1
    ok = abi.TrackUndistortInC()
    camc = eng.camera(cam)
    ok.camera, ok.num_points, ok.time = C.pointer(camc), 30, 9.0
    ok.pts, ok.ids = p1.ctypes.data_as(fp), ids.ctypes.data_as(C.POINTER(C.c_int))
    for k in range(3):  # a null output with N > 0
        args = list(o)
        args[k] = None
        assert eng.lib.lfvio_track_undistort(eng.ctx, C.byref(ok), args[0], args[1], args[2], None) == -1, k
    assert all(np.all(a == 7.5) for a in outs[:3]) and np.all(outs[3] == 77)
    got = eng.track_undistort(cam, p1, ids, 1.25)
    for key in ("un_pts", "un_pts_3d", "velocity_3d", "matched"):
        assert same(got[key], want[key]), key


def test_repeatable_whatever_the_size_and_the_index(eng):
    """Test 7a: a point's outputs depend neither on N nor on its index nor on the run."""
    cam = tr.SKEW
    cur, forw = tr.make_matches(71, cam, 700)
    s = tr.make_samples(72, 700, 100)
    a = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    b = eng.track_reject(cam, cur, forw, s, want_bearings=True)
    for key in ("mask", "E", "bearing_cur", "bearing_forw"):
        assert same(a[key], b[key]), key
    assert (a["status"], a["best_sample"], a["num_inliers"], a["best_score"]) == (b["status"], b["best_sample"], b["num_inliers"], b["best_score"])
    perm = np.random.default_rng(73).permutation(700)[:77]
    c = eng.track_reject(cam, cur[perm], forw[perm], tr.make_samples(74, 77, 3), want_bearings=True)
    assert same(c["bearing_cur"], a["bearing_cur"][perm]) and same(c["bearing_forw"], a["bearing_forw"][perm])
    ids = np.arange(700, dtype=np.int32)
    eng.track_reset()
    eng.track_undistort(cam, cur, ids, 1.0)
    u = eng.track_undistort(cam, forw, ids, 1.1)
    eng.track_reset()
    eng.track_undistort(cam, cur[::-1], ids[::-1], 1.0)
    v = eng.track_undistort(cam, forw[perm], ids[perm], 1.1)
    for key in ("un_pts", "un_pts_3d", "velocity_3d"):
        assert same(v[key], u[key][perm]), key
    assert same(v["matched"], (699 - perm).astype(np.int32)) and u["velocity_3d"].any()


def test_beside_an_optimization_in_flight(eng):
    """Test 7b: between lfvio_batch_optimize_begin and _finish — the optimization's state and prior are the bits of the call with
    nothing in between, and both tracker calls give the bits of an idle context."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    w = synth.make_window(0, 300)
    cam = tr.PAL
    cur, forw = tr.make_matches(81, cam, 150)
    s = tr.make_samples(82, 150, 100)
    ids = np.arange(150, dtype=np.int32)

    def tracker_calls(e):
        e.track_reset()
        r = e.track_reject(cam, cur, forw, s, want_bearings=True)
        e.track_undistort(cam, cur, ids, 3.0)
        return r, e.track_undistort(cam, forw, ids, 3.05)

    alone_r, alone_u = tracker_calls(eng)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    sol0, prior0, _ = split(Engine(0), None)
    sol1, prior1, (r, u) = split(Engine(0), tracker_calls)
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    for key in ("mask", "E", "bearing_cur", "bearing_forw"):
        assert same(r[key], alone_r[key]), key
    assert (r["status"], r["best_sample"], r["num_inliers"]) == (alone_r["status"], alone_r["best_sample"], alone_r["num_inliers"])
    for key in ("un_pts", "un_pts_3d", "velocity_3d", "matched"):
        assert same(u[key], alone_u[key]), key
