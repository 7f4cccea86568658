"""lfvio_track_batch_* on the device against the library itself: slot i of a batch equals a FRESH context given slot i's active frames,
in order, through lfvio_track_frame_message with the same mask and CLAHE setting.  Every comparison is tobytes() equality: the table,
the outputs of undistortedPoints, every scalar, the rejection record, LfvioGftOut and the message rows.  No tolerance anywhere.

The images are 161 x 123: klt_ref.texture(seed), one seed per slot, moved as tests/test_tracker_chain.py moves its texture, with that
file's CAM, MAX_CNT 40, MIN_DIST 10 and S = 100.

  1  three slots, six frames each
  2  unlike slots in one call: publish off in slot 1 on frames 2 and 4, slot 2 idle on frame 3, another camera in slot 1, annulus
     masks of different radii, CLAHE (3.0, 8 x 8) on
  3  the small and empty cases beside full ones: a grey first frame in slot 0, grey frames after textured ones in slot 1, then the
     whole batch at max_count = 6 (n1 < 8, rejection status 2 in every slot)
  4  one slot is the single call; the two routes interleaved on one engine leave each other's resident state alone
  5  reset of one slot, reserve again, reserve(0)
  6  refused calls: outputs and messages untouched (sentinel bytes), and the next valid call equals that of a run that never saw them
  7  repeatability, and a run beside an optimization in flight"""
import ctypes as C

import numpy as np
import pytest

import gft_ref
import klt_ref
from test_tracker_chain import CAM, FRAMES, H, MAX_CNT, MIN_DIST, W, same

pytestmark = pytest.mark.gpu

S = 100
KW = dict(max_count=MAX_CNT, min_distance=MIN_DIST, mask_radius=MIN_DIST)
TABLE = ("pts", "ids", "track_cnt", "un_pts", "un_pts_3d", "velocity_3d")
SCALARS = ("num_points", "num_new", "levels_used", "num_tracked", "num_after_reject", "num_rows")
SEEDS = (5, 6, 7)
CAM_B = dict(CAM, cx=83.5, cy=58.0, poly=tuple(c * (1.0 + 0.03 * i) for i, c in enumerate(CAM["poly"])))
GREY = np.full((H, W), 117, np.uint8)


def sequence(seed):
    f = klt_ref.texture(seed)
    out = []
    for k in range(FRAMES):
        _, inv = klt_ref.warp(W, H, shift=(1.5 * k, -0.75 * k), scale=0.004 * k, angle=0.006 * k)
        out.append(klt_ref.render(f, W, H, inv))
    return out


@pytest.fixture(scope="module")
def seqs():
    return [sequence(s) for s in SEEDS]


def words(slot, k):
    return np.random.default_rng([k, 41, slot]).integers(0, 2 ** 32, (S, 8), dtype=np.uint64).astype(np.uint32)


def when(k):
    return 20.0 + 0.05 * k


def entry(slot, k, img, cam=CAM, publish=True):
    return dict(img=img, time=when(k), cam=cam, publish=publish, words=words(slot, k))


def alone(entries, mask=None, clahe=False, kw=KW):
    """The entries of one slot (None: idle, skipped) through lfvio_track_frame_message on a fresh context."""
    from lfvio.engine import Engine

    e = Engine(0)
    try:
        if clahe:
            e.clahe_set(3.0, (8, 8))
        if mask is not None:
            e.gft_set_mask(mask)
        return [None if f is None else e.track_frame_message(f["img"], f["time"], f["cam"], publish=f["publish"], words=f["words"], **kw) for f in entries]
    finally:
        e.close()


def record(r):
    """Everything one slot's frame gave, as bytes."""
    rj, dt = r["reject"], r["detect"]
    parts = [np.ascontiguousarray(r[key]).tobytes() for key in TABLE] + [np.ascontiguousarray(r["rows"]).tobytes()]
    parts.append(repr([r[key] for key in SCALARS] + [rj["status"], rj["best_sample"], rj["num_inliers"], dt["num_kept"], dt["num_corners"],
                                                     dt["num_candidates"]]).encode())
    parts += [np.float64(rj["best_score"]).tobytes(), np.ascontiguousarray(rj["E"]).tobytes(), np.float64(dt["max_response"]).tobytes()]
    return parts


def agree(got, want, tag):
    assert got["rc"] == 0 and want["rc"] == 0, tag
    for key in TABLE + ("rows",):
        assert same(got[key], want[key]), (tag, key)
    assert record(got) == record(want), tag


def idle(r):
    return r["num_points"] == 0 and r["num_rows"] == 0 and r["reject"]["status"] == 0 and not r["reject"]["E"].any() and r["levels_used"] == 0


def batch(eng, columns, **kw):
    """columns[slot][k]: an entry or None; one batch call per k.  Returns results[slot][k]."""
    out = [[] for _ in columns]
    for k in range(len(columns[0])):
        res = eng.track_batch_frame([col[k] for col in columns], **dict(KW, **kw))
        for slot, r in enumerate(res):
            out[slot].append(r)
    return out


def plain(eng, slots):
    eng.track_batch_reserve(slots)
    eng.track_batch_clahe(None)


def three(seqs, frames=range(FRAMES)):
    return [[entry(slot, k, seqs[slot][k]) for k in frames] for slot in range(3)]


@pytest.fixture(scope="module")
def refs(seqs):
    """The three plain sequences, each on a context of its own: computed once, shared, never changed."""
    return [alone(col) for col in three(seqs)]


def test_three_slots_six_frames(eng, seqs, refs):
    """Test 1."""
    plain(eng, 3)
    got = batch(eng, three(seqs))
    for slot in range(3):
        for k in range(FRAMES):
            agree(got[slot][k], refs[slot][k], (slot, k))
        assert got[slot][0]["num_points"] >= 20 and got[slot][-1]["num_rows"] >= 8 and got[slot][-1]["velocity_3d"].any()
        assert sum(r["reject"]["status"] == 0 for r in got[slot]) >= 3 and any(r["num_new"] > 0 for r in got[slot][1:])
    assert record(got[0][3]) != record(got[1][3]) != record(got[2][3])  # three streams, not one


def test_unlike_slots_in_one_call(eng, seqs):
    """Test 2."""
    masks = [gft_ref.annulus_mask(W, H, 80, 61, r_out, r_in) for r_out, r_in in ((70, 10), (60, 15), (50, 5))]
    cams = (CAM, CAM_B, CAM)
    cols = [[entry(slot, k, seqs[slot][k], cam=cams[slot], publish=not (slot == 1 and k in (2, 4))) for k in range(FRAMES)] for slot in range(3)]
    cols[2][3] = None
    try:
        plain(eng, 3)
        eng.track_batch_clahe(3.0, (8, 8))
        for slot in range(3):
            eng.track_batch_set_mask(slot, masks[slot])
        got = batch(eng, cols)
        for slot in range(3):
            want = alone(cols[slot], mask=masks[slot], clahe=True)
            for k in range(FRAMES):
                if cols[slot][k] is None:
                    assert idle(got[slot][k]), (slot, k)
                else:
                    agree(got[slot][k], want[k], (slot, k))
        assert got[1][2]["num_new"] == 0 and got[1][2]["num_rows"] == 0 and got[1][2]["num_points"] == got[1][2]["num_tracked"] > 8
        assert got[2][4]["num_points"] >= 10 and got[2][4]["velocity_3d"].any()  # the frame behind the idle one: a context that never saw frame 3
        # the camera, the masks and the setting did count
        unmasked = alone(cols[0][:1])[0]
        assert not same(unmasked["pts"], got[0][0]["pts"])
        assert not same(alone(cols[1][:1], mask=masks[1], clahe=True)[0]["un_pts"], alone([dict(cols[1][0], cam=CAM)], mask=masks[1], clahe=True)[0]["un_pts"])
    finally:
        eng.track_batch_clahe(None)


def test_small_and_empty_cases_beside_full_ones(eng, seqs, refs):
    """Test 3."""
    plain(eng, 3)
    cols = [[entry(0, k, img) for k, img in enumerate([GREY, seqs[0][0], seqs[0][1], seqs[0][2]])],
            [entry(1, k, img) for k, img in enumerate([seqs[1][0], seqs[1][1], GREY, GREY])],
            [entry(2, k, seqs[2][k]) for k in range(4)]]
    got = batch(eng, cols)
    for slot in range(2):
        want = alone(cols[slot])
        for k in range(4):
            agree(got[slot][k], want[k], ("grey", slot, k))
    for k in range(4):
        agree(got[2][k], refs[2][k], ("full beside grey", k))
    assert got[0][0]["num_points"] == 0 and got[0][0]["reject"]["status"] == 2 and got[0][1]["num_points"] >= 20
    assert got[1][1]["num_points"] >= 20 and got[1][2]["detect"]["num_corners"] == 0
    assert (got[1][3]["num_tracked"], got[1][3]["num_points"], got[1][3]["num_new"]) == (0, 0, 0)  # the table emptied on the device
    # the whole batch at max_count = 6
    plain(eng, 3)
    small = dict(KW, max_count=6)
    cols = three(seqs, range(4))
    got = batch(eng, cols, max_count=6)
    for slot in range(3):
        want = alone(cols[slot], kw=small)
        for k in range(4):
            agree(got[slot][k], want[k], ("max_count 6", slot, k))
            r = got[slot][k]
            assert r["num_tracked"] < 8 and r["reject"]["status"] == 2 and r["num_after_reject"] == r["num_tracked"] and r["num_points"] <= 6
    assert got[0][1]["num_tracked"] >= 3


def test_one_slot_is_the_single_call(eng, seqs, refs):
    """Test 4: slot 0 of a batch of one takes sequence 0 while the same engine's single route takes sequence 1, frame about."""
    plain(eng, 1)
    eng.clahe_set(None)
    eng.gft_set_mask(None)
    eng.track_frame_reset()
    for k in range(FRAMES):
        b = eng.track_batch_frame([entry(0, k, seqs[0][k])], **KW)[0]
        f = entry(1, k, seqs[1][k])
        s = eng.track_frame_message(f["img"], f["time"], f["cam"], publish=True, words=f["words"], **KW)
        agree(b, refs[0][k], ("batch of one", k))
        agree(s, refs[1][k], ("single beside the batch", k))
    # the single route's resident image is its own last frame, not the batch's
    assert same(eng.klt_level(0), seqs[1][FRAMES - 1])
    # and the single route on the SAME engine, given the batch's sequence, gives the batch's bits
    eng.track_frame_reset()
    for k in range(2):
        f = entry(0, k, seqs[0][k])
        agree(eng.track_frame_message(f["img"], f["time"], f["cam"], publish=True, words=f["words"], **KW), refs[0][k], ("single", k))
    eng.track_frame_reset()


def test_reset_and_reserve(eng, seqs, refs):
    """Test 5."""
    plain(eng, 3)
    cols = three(seqs)
    first = batch(eng, [col[:3] for col in cols])
    eng.track_batch_reset(1)
    rest = batch(eng, [col[3:] for col in cols])
    again = alone(cols[1][3:])
    for k in range(3):
        agree(rest[0][k], refs[0][3 + k], ("unbroken", 0, k))
        agree(rest[2][k], refs[2][3 + k], ("unbroken", 2, k))
        agree(rest[1][k], again[k], ("after reset", k))
    assert rest[1][0]["num_new"] == rest[1][0]["num_points"] and rest[1][0]["ids"].min() == 0 and first[1][2]["num_points"] >= 20
    eng.track_batch_reserve(3)  # again: every slot empty
    got = batch(eng, [col[:2] for col in cols])
    for slot in range(3):
        for k in range(2):
            agree(got[slot][k], refs[slot][k], ("reserved again", slot, k))
    eng.track_batch_reserve(0)
    r = eng.track_batch_frame([cols[0][0]], check=False, **KW)
    assert r[0]["rc"] == -1
    assert eng.track_batch_reset(-1, check=False) == -1 and eng.track_batch_set_mask(0, None, check=False) == -1


def sentinels(n):
    from lfvio import abi

    out = []
    for _ in range(n):
        arrays = dict(pts=np.full((4096, 2), 7.5, np.float32), ids=np.full(4096, 77, np.int32), track_cnt=np.full(4096, 77, np.int32),
                      un_pts=np.full((4096, 2), 7.5, np.float32), un_pts_3d=np.full((4096, 3), 7.5, np.float32),
                      velocity_3d=np.full((4096, 3), 7.5, np.float32))
        o = abi.TrackFrameOutC()
        C.memset(C.byref(o), 0x5A, C.sizeof(o))
        out.append((arrays, o, np.full((4096, 9), 7.5, np.float32)))
    return out


def untouched(bufs, res):
    from lfvio import abi

    head = abi.TrackFrameOutC.pts.offset
    for (arrays, o, rows), r in zip(bufs, res):
        if bytes(o)[:head] != b"\x5a" * head or r["msg_num_rows"] != -77 or not np.all(rows == 7.5):
            return False
        if not all(np.all(a == (77 if a.dtype == np.int32 else 7.5)) for a in arrays.values()):
            return False
    return True


def test_refused_calls_leave_everything_alone(eng, seqs, refs):
    """Test 6."""
    plain(eng, 3)
    cols = three(seqs)
    batch(eng, [col[:2] for col in cols])
    count = max(refs[slot][1]["num_points"] for slot in range(3))
    assert count >= 20
    good = [col[2] for col in cols]
    nan = float("nan")
    # (what the call is given, the shared parameters)
    unlike = [dict(width=160), dict(height=122), dict(win_size=39), dict(max_level=2), dict(max_iterations=29), dict(epsilon=0.02),
              dict(min_eig_threshold=2e-4), dict(border=2), dict(max_count=MAX_CNT + 1), dict(quality_level=0.02), dict(min_distance=MIN_DIST + 1),
              dict(mask_radius=MIN_DIST + 1), dict(num_samples=S - 1), dict(capacity=4095)]
    assert len(unlike) == 14
    refused = [([good[0], dict(good[1], params=p), good[2]], {}) for p in unlike]
    refused += [([good[0], good[1], dict(good[2], params=p)], {}) for p in (dict(win_size=4), dict(max_level=6), dict(epsilon=nan), dict(num_samples=0))]
    refused += [([good[0], dict(good[1], cam=None), good[2]], {}), ([dict(good[0], words=None, params=dict(num_samples=S)), good[1], good[2]], {}),
                ([good[0], good[1], dict(good[2], time=nan)], {}), ([good[0], dict(good[1], cam=dict(CAM, model=1)), good[2]], {})]
    refused += [(good, dict(max_count=10, capacity=count - 1)), (good, dict(capacity=MAX_CNT - 1)), (good, dict(capacity=4097))]
    refused += [(good[:2], {}), (good, dict(count=2)), (good, dict(count=4)), (good, dict(count=0))]
    n = 0
    for frames, extra in refused:
        extra = dict(extra)
        cnt = extra.pop("count", None)
        bufs = sentinels(len(frames))
        res = eng.track_batch_frame(frames, count=cnt, buffers=bufs, check=False, **dict(KW, **extra))
        assert res[0]["rc"] == -1, (n, extra)
        assert untouched(bufs, res), (n, extra)
        n += 1
    # a null array in one slot's out; a base mask of another size in one publishing slot
    bufs = sentinels(3)
    keep, bufs[1][0]["un_pts"] = bufs[1][0]["un_pts"], None
    res = eng.track_batch_frame(good, buffers=bufs, check=False, **KW)
    bufs[1][0]["un_pts"] = keep
    assert res[0]["rc"] == -1 and untouched(bufs, res)
    eng.track_batch_reset(2)
    eng.track_batch_set_mask(2, np.full((H, W + 3), 255, np.uint8))
    bufs = sentinels(3)
    res = eng.track_batch_frame(good, buffers=bufs, check=False, **KW)
    assert res[0]["rc"] == -1 and untouched(bufs, res)
    eng.track_batch_set_mask(2, None)
    # the other calls
    assert eng.track_batch_reserve(65, check=False) == -1 and eng.track_batch_reserve(-1, check=False) == -1
    assert eng.track_batch_reset(3, check=False) == -1 and eng.track_batch_reset(-2, check=False) == -1
    assert eng.track_batch_set_mask(3, np.full((H, W), 255, np.uint8), check=False) == -1
    assert eng.track_batch_set_mask(0, np.full((H, W + 1), 255, np.uint8), check=False) == -1  # not slot 0's resident image's size
    assert eng.track_batch_set_mask(-1, np.full((8, 8), 255, np.uint8), check=False) == -1
    assert eng.track_batch_clahe(3.0, (17, 8), check=False) == -1
    lib = eng.lib
    assert lib.lfvio_track_batch_frame(eng.ctx, 3, None, None, None) == -1 and lib.lfvio_track_batch_frame(None, 3, None, None, None) == -1
    assert lib.lfvio_track_batch_reserve(None, 3) == -1 and lib.lfvio_track_batch_reset(None, 0) == -1
    assert n >= 29
    # an all-idle call is accepted and moves nothing
    res = eng.track_batch_frame([None, None, None], **KW)
    assert all(r["rc"] == 0 and idle(r) for r in res)
    # nothing resident moved in slots 0 and 1 (slot 2 was reset above: it starts again)
    res = eng.track_batch_frame(good, **KW)
    agree(res[0], refs[0][2], "slot 0 behind the refused calls")
    agree(res[1], refs[1][2], "slot 1 behind the refused calls")
    agree(res[2], alone([good[2]])[0], "slot 2 behind its reset")
    assert res[0]["velocity_3d"].any()


def test_repeatable_and_beside_an_optimization_in_flight(eng, seqs, refs):
    """Test 7."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    cols = [col[:3] for col in three(seqs)]

    def run(e):
        e.track_batch_reserve(3)
        return [record(r) for col in batch(e, cols) for r in col]

    first = run(eng)
    assert run(eng) == first and first == [record(r) for slot in range(3) for r in refs[slot][:3]]
    w = synth.make_window(0, 300)

    def split(e, between):
        try:
            e.batch_reserve(1, w.N, w.M)
            e.batch_upload(0, w)
            sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
            res = between(e) if between else None
            return sol, e.optimize_finish(), res
        finally:
            e.close()

    sol0, prior0, _ = split(Engine(0), None)
    sol1, prior1, recs = split(Engine(0), run)
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert recs == first
