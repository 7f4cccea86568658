"""The batched tracker on the EXPANDED image (lfvio_track_batch_map, lfvio_track_batch_source, k_remap_gray_b).  The
contract, bit for bit and without a tolerance anywhere: after any sequence of batch calls, slot i's outputs, message and every level
of its resident pyramid are those of a FRESH context given lfvio_remap_build with slot i's recipe, lfvio_image_format_set and
lfvio_track_source_set with the batch's settings, and slot i's active frames through lfvio_track_frame_message.

Sources are 161 x 123 noise with a padded odd step, or the 320 x 240 frames of trace.make_image_stream(scale=4); outputs are 131 x 67
(8777 pixels, 1 mod 4: the last lane's tail) and 128 x 64.  The three maps of a batch: equirectangular through the PAL camera,
perspective through the pinhole camera behind the shifted M, equirectangular through the PAL camera at another scale.

  1  level 0 per slot: after one batch frame every slot's level 0 equals tracksource_ref.level0 of its own map, for mono8, bgr8, bgra8
     and mono16 of both byte orders with odd steps; every map is first shown, on the CPU, to have inside AND outside entries
  2  the contract: six rendered frames, CLAHE off and on, bgr8 at 131 x 67 and mono16 at 128 x 64; slot 1 idle in frames 2 and 4,
     slot 2 not publishing in frame 3
  3  slot = -1: one lfvio_track_batch_map for 64 slots, one mono8 frame at 128 x 64; slots 0, 31 and 63 equal one fresh context
  4  the geometry changes: the step through lfvio_track_batch_format between frames, slot 1's map rebuilt with another recipe of the
     same size, lfvio_remap_build / lfvio_remap_apply of another size on the same context in between — everybody still equals their
     own reference
  5  refusals (LFVIO_ERR_ARG with a message, sentinel-filled outputs untouched): an active slot without a map, a map of another size,
     a step one byte short of the source's row, source sides of 15 and 8193; the next good call gives the bytes of slots that never
     saw a refused one; reserve drops the maps, reset keeps them; lfvio_track_batch_source(NULL) gives plain batched frames
  6  the host route: lfvio_host_track_traces over three rendered recordings of 12, 12 and 9 frames with `expand` on writes, byte for
     byte, the three files lfvio_host_track_trace writes for each alone; a fourth recording of another image size makes the call
     fail and write nothing
  7  the host route with `expand` off: three recordings of 10, 10 and 7 frames at 160 x 120 with the annulus, CLAHE, frames that are
     tracked only and one restart, against each alone and against tests/node_ref.Gate's counts"""
import os

import numpy as np
import pytest

import equirect_ref as er
import image_ref as ir
import project_ref as pr
from test_track_batch import sentinels, untouched
from test_track_source_gpu import FH, FW, SH, SW, Map, arm, everything, kw, last_error, levels, odd_step, words
from test_tracker_chain import same

pytestmark = pytest.mark.gpu

OUT = ((131, 67), (128, 64))
KINDS = ("equirect", "perspective", "equirect2")
ERR_ARG = -1


class Recipe(Map):
    """test_track_source_gpu.Map with a third kind (the PAL camera at another scale) and the numpy maps made when first asked for."""

    def __init__(self, kind, size, src_size):
        self.size, self.src_size, self._xy = size, src_size, None
        if kind == "perspective":
            self.cam, self.kind = pr.small(pr.CAMS["EUROC_ND"][0], pr.CAMS["EUROC_ND"][1][0] / src_size[0]), pr.MAP_PERSPECTIVE
            self.M = pr.K_inverse(self.cam) @ np.array([[1.0, 0.0, -20.0], [0.0, 1.0, 70.0], [0.0, 0.0, 1.0]])
        else:
            scale = 1.0 if kind == "equirect" else 1.15
            self.cam, self.kind, self.M = pr.small(pr.PAL, scale * pr.CAMS["PAL"][1][0] / src_size[0]), pr.MAP_EQUIRECT, None
        # the camera of the image that is TRACKED
        self.track_cam = er.camera(*size) if self.kind == pr.MAP_EQUIRECT else dict(self.cam)

    def _maps(self):
        if self._xy is None:
            self._xy = pr.build(self.cam, self.kind, self.size[0], self.size[1], self.M)
        return self._xy

    x = property(lambda self: self._maps()[0])
    y = property(lambda self: self._maps()[1])

    def batch(self, e, slot, check=True):
        return e.track_batch_map(slot, self.cam, self.kind, self.size[0], self.size[1], self.M, check=check)


@pytest.fixture(scope="module")
def recipes():
    """Computed once, shared, never changed."""
    return {(kind, size, src): Recipe(kind, size, src) for kind in KINDS for size in OUT for src in ((SW, SH), (FW, FH))}


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """Six 320 x 240 frames of the rendered stream: made once, shared, never changed."""
    from lfvio import trace

    p = str(tmp_path_factory.mktemp("trackbatchsource") / "s.lfvt")
    made = trace.make_image_stream(p, seed=2, n_frames=6, scale=4)
    assert (made["width"], made["height"]) == (FW, FH)
    return [img for _, img in trace.read_trace(p)["raw_images"]]


def three(recipes, size, src):
    return [recipes[kind, size, src] for kind in KINDS]


def arm_batch(e, ms, code, step, src_size, clahe=False, together=False):
    e.track_batch_reserve(len(ms))
    e.track_batch_clahe(3.0, (8, 8)) if clahe else e.track_batch_clahe(None)
    e.track_batch_format(code, step)
    e.track_batch_source(*src_size)
    if together:
        ms[0].batch(e, -1)
    else:
        for slot, m in enumerate(ms):
            m.batch(e, slot)


def disarm_batch(e):
    e.track_batch_source(None)
    e.track_batch_format(None)
    e.track_batch_clahe(None)
    e.track_batch_reserve(0)


def slot_levels(e, slot):
    out = []
    for k in range(6):
        px = e.track_batch_level(slot, k, check=False)
        if px is None:
            break
        out.append(px.tobytes())
    return out


def entry(m, k, rows, publish=True, slot=0):
    return dict(img=rows, time=5.0 + 0.1 * k, cam=m.track_cam, publish=publish, words=words(10 * k + slot))


def alone(m, code, step, entries, clahe=False):
    """One slot's entries (None: idle, skipped) on a fresh context of its own, the second side of the contract.  An entry may carry
    `map` (a recipe built in front of it) and `step` (the format set in front of it).  -> per entry (everything, the pyramid)."""
    from lfvio.engine import Engine

    e = Engine(0)
    try:
        arm(e, m, code, step, clahe)
        out = []
        for f in entries:
            if f is None:
                out.append(None)
                continue
            if "map" in f:
                f["map"].build(e)
            if "step" in f:
                e.image_format(code, f["step"])
            r = e.track_frame_message(f["img"], f["time"], f["cam"], publish=f["publish"], words=f["words"], **kw(m.size))
            out.append((everything(r), levels(e), r))
        return out
    finally:
        e.close()


def call(f):
    return None if f is None else {k: v for k, v in f.items() if k not in ("map", "step")}


# ---- 1
@pytest.mark.parametrize("size", OUT)
def test_level0_per_slot(eng, recipes, size):
    ms = three(recipes, size, (SW, SH))
    W, H = size
    try:
        for code in (ir.MONO8, ir.BGR8, ir.BGRA8, ir.MONO16, ir.MONO16_BE):
            step = odd_step(SW, code)
            assert step % 2 == 1
            for m in ms:
                off = pr.offsets(m.x, m.y, SW, SH, step, ir.BPP[code])
                assert (off >= 0).sum() > 0 and (off < 0).sum() > 0  # the gather path and the select path both run
            rows = [pr.noise_image(40 + 3 * code + slot, SW, SH, code, step) for slot in range(3)]
            arm_batch(eng, ms, code, step, (SW, SH))
            res = eng.track_batch_frame([entry(m, 0, r, slot=slot) for slot, (m, r) in enumerate(zip(ms, rows))], **kw(size))
            want = [m.level0(r, code, step) for m, r in zip(ms, rows)]
            for slot in range(3):
                got = eng.track_batch_level(slot, 0)
                assert res[slot]["rc"] == 0 and got.shape == (H, W) and same(got, want[slot]), (size, code, slot)
            assert len({w.tobytes() for w in want}) == 3
    finally:
        disarm_batch(eng)


# ---- 2
@pytest.mark.parametrize("clahe", [False, True])
@pytest.mark.parametrize("code,size", [(ir.BGR8, (131, 67)), (ir.MONO16, (128, 64))])
def test_contract(eng, recipes, frames, code, size, clahe):
    ms = three(recipes, size, (FW, FH))
    step = odd_step(FW, code)
    rows = [ir.from_gray(g, code, step, seed=30 + k) for k, g in enumerate(frames)]
    assert len(rows) == 6
    cols = [[entry(m, k, rows[k], publish=not (slot == 2 and k == 3), slot=slot) for k in range(6)] for slot, m in enumerate(ms)]
    cols[1][2] = cols[1][4] = None
    want = [alone(m, code, step, col, clahe) for m, col in zip(ms, cols)]
    try:
        arm_batch(eng, ms, code, step, (FW, FH), clahe)
        for k in range(6):
            res = eng.track_batch_frame([col[k] for col in cols], **kw(size))
            for slot in range(3):
                if cols[slot][k] is None:
                    assert res[slot]["num_points"] == 0 and res[slot]["num_rows"] == 0
                    continue
                assert everything(res[slot]) == want[slot][k][0], (slot, k)
                lv = slot_levels(eng, slot)
                assert lv == want[slot][k][1] and len(lv) >= 2, (slot, k)
        for slot in range(3):
            r = res[slot]
            print(f"slot {slot}: {r['num_points']} points, {r['num_tracked']} tracked, {r['num_rows']} rows")
            assert r["num_points"] >= 10 and r["velocity_3d"].any(), slot  # not a comparison of empty tables
        assert len({tuple(want[slot][5][0]) for slot in range(3)}) == 3  # three streams, not one
        if not clahe:  # level 0 is the grey image of the expanded one
            assert slot_levels(eng, 0)[0] == ms[0].level0(rows[5], code, step).tobytes()
    finally:
        disarm_batch(eng)


# ---- 3
def test_every_slot_in_one_build(eng, recipes, frames):
    size, code = (128, 64), ir.MONO8
    m = recipes["equirect", size, (FW, FH)]
    f = entry(m, 0, frames[0])
    want = alone(m, code, 0, [f])[0]
    try:
        arm_batch(eng, [m] * 64, code, 0, (FW, FH), together=True)
        res = eng.track_batch_frame([f] * 64, **kw(size))
        for slot in (0, 31, 63):
            assert everything(res[slot]) == want[0] and slot_levels(eng, slot) == want[1], slot
        assert res[63]["num_points"] >= 10
    finally:
        disarm_batch(eng)


# ---- 4
def test_geometry_changes(eng, recipes, frames):
    size, code = (128, 64), ir.BGR8
    ms = three(recipes, size, (FW, FH))
    other = recipes["equirect", (131, 67), (SW, SH)]  # the context's OWN resident map: another size, another source
    steps = [odd_step(FW, code), 3 * FW, 3 * FW + 8, odd_step(FW, code), 3 * FW + 8, 3 * FW]
    rows = [ir.from_gray(g, code, st, seed=50 + k) for k, (g, st) in enumerate(zip(frames, steps))]
    noise = pr.noise_image(77, SW, SH, ir.MONO16, 2 * SW + 3)
    cols = [[dict(entry(m, k, rows[k], slot=slot), step=steps[k]) for k in range(6)] for slot, m in enumerate(ms)]
    # slot 1's recipe changes in front of frames 2 and 4: to slot 2's, and back
    cols[1][2]["map"], cols[1][4]["map"] = ms[2], ms[1]
    cols[1][2]["cam"] = cols[1][3]["cam"] = ms[2].track_cam
    want = [alone(m, code, steps[0], col) for m, col in zip(ms, cols)]
    try:
        arm_batch(eng, ms, code, steps[0], (FW, FH))
        for k in range(6):
            eng.track_batch_format(code, steps[k])
            if "map" in cols[1][k]:
                cols[1][k]["map"].batch(eng, 1)
            # the context's own maps, built and used between every two batch frames
            other.build(eng)
            o = eng.remap_apply(noise, SW, SH, other.size, encoding=ir.MONO16, step=2 * SW + 3)
            assert same(o, pr.remap(noise, other.x, other.y, SW, SH, ir.MONO16, 2 * SW + 3)), k
            res = eng.track_batch_frame([call(col[k]) for col in cols], **kw(size))
            for slot in range(3):
                assert everything(res[slot]) == want[slot][k][0] and slot_levels(eng, slot) == want[slot][k][1], (slot, k)
            # ... and behind a batch frame the context's integer map is still its own
            o = eng.remap_apply(noise, SW, SH, other.size, encoding=ir.MONO16, step=2 * SW + 3)
            assert same(o, pr.remap(noise, other.x, other.y, SW, SH, ir.MONO16, 2 * SW + 3)), k
        assert all(res[slot]["num_points"] >= 10 for slot in range(3))
    finally:
        eng.remap_reset()
        disarm_batch(eng)


# ---- 5
def refused(e, frames_in, size, why):
    bufs = sentinels(len(frames_in))
    res = e.track_batch_frame(frames_in, buffers=bufs, check=False, **kw(size))
    assert res[0]["rc"] == ERR_ARG and why in last_error(e) and untouched(bufs, res), (why, last_error(e))


def test_refusals(eng, recipes, frames):
    from lfvio.engine import Engine

    size, code = (131, 67), ir.BGR8
    ms, wrong = three(recipes, size, (FW, FH)), recipes["equirect", (128, 64), (FW, FH)]
    step = odd_step(FW, code)
    rows = [ir.from_gray(g, code, step, seed=70 + k) for k, g in enumerate(frames[:4])]
    cols = [[entry(m, k, rows[k], slot=slot) for k in range(4)] for slot, m in enumerate(ms)]
    want = [alone(m, code, step, col) for m, col in zip(ms, cols)]  # the contexts that never see a refused call
    good = lambda k: [col[k] for col in cols]

    def agrees(res, k, slots=(0, 1, 2)):
        for slot in slots:
            assert everything(res[slot]) == want[slot][k][0] and slot_levels(eng, slot) == want[slot][k][1], (slot, k)

    try:
        # no map: slot 1 never built one; idle, it needs none
        eng.track_batch_reserve(3)
        eng.track_batch_clahe(None)
        eng.track_batch_format(code, step)
        eng.track_batch_source(FW, FH)
        ms[0].batch(eng, 0), ms[2].batch(eng, 2)
        refused(eng, good(0), size, "no map")
        res = eng.track_batch_frame([cols[0][0], None, cols[2][0]], **kw(size))
        agrees(res, 0, (0, 2))
        ms[1].batch(eng, 1)
        eng.track_batch_reset(-1)  # the slots start again; reset keeps the maps
        agrees(eng.track_batch_frame(good(0), **kw(size)), 0)
        # the set call refuses sides of 15 and 8193; the setting stays
        for side in (15, 8193):
            assert eng.track_batch_source(side, FH, check=False) == ERR_ARG and "[16, 8192]" in last_error(eng)
            assert eng.track_batch_source(FW, side, check=False) == ERR_ARG and "[16, 8192]" in last_error(eng)
        assert eng.lib.lfvio_track_batch_source(None, None) == ERR_ARG and eng.lib.lfvio_track_batch_map(None, 0, None) == ERR_ARG
        assert eng.track_batch_map(3, check=False) == ERR_ARG and ms[0].batch(eng, -2, check=False) == ERR_ARG
        assert eng.track_batch_map(0, ms[0].cam, 7, 131, 67, check=False) == ERR_ARG and eng.track_batch_map(0, ms[0].cam, pr.MAP_EQUIRECT, 15, 67, check=False) == ERR_ARG
        # a map of another size in slot 2
        wrong.batch(eng, 2)
        refused(eng, good(1), size, "another size")
        ms[2].batch(eng, 2)
        # a step one byte short of the source's row: enough for the 131 pixels tracked, not for the 320 of the source
        eng.track_batch_format(code, 3 * FW - 1)
        assert 3 * FW - 1 > 3 * size[0]
        refused(eng, good(1), size, "step below width")
        eng.track_batch_format(code, step)
        # a forgotten map
        eng.track_batch_map(1)
        refused(eng, good(1), size, "no map")
        ms[1].batch(eng, 1)
        # the next good calls give the bytes of slots that never saw a refused one
        for k in (1, 2):
            res = eng.track_batch_frame(good(k), **kw(size))
            agrees(res, k)
        assert all(res[slot]["num_points"] >= 10 for slot in range(3))
        # lfvio_track_batch_level's own refusals
        assert eng.track_batch_level(3, 0, check=False) is None and "slot outside" in last_error(eng)
        assert eng.track_batch_level(-1, 0, check=False) is None and "slot outside" in last_error(eng)
        assert eng.track_batch_level(0, 9, check=False) is None and "not built" in last_error(eng)
        # reserve drops the maps (and the setting, which is the batch's, stays)
        eng.track_batch_reserve(3)
        refused(eng, good(0), size, "no map")
        for slot, m in enumerate(ms):
            m.batch(eng, slot)
        agrees(eng.track_batch_frame(good(0), **kw(size)), 0)
        # off again: plain batched frames, the images are the tracked images
        eng.track_batch_source(None)
        eng.track_batch_format(None)
        eng.track_batch_reset(-1)
        plain = [ms[0].level0(rows[k], code, step) for k in range(3)]
        got = [eng.track_batch_frame([dict(cols[0][k], img=plain[k]), None, None], **kw(size))[0] for k in range(3)]
        twin = Engine(0)
        try:
            ref = [twin.track_frame_message(plain[k], cols[0][k]["time"], cols[0][k]["cam"], publish=True, words=cols[0][k]["words"], **kw(size)) for k in range(3)]
        finally:
            twin.close()
        for k in range(3):
            assert everything(got[k]) == everything(ref[k]), k
        assert got[2]["num_points"] >= 10 and same(eng.track_batch_level(0, 0), plain[2])
    finally:
        disarm_batch(eng)


# ---- 6
def test_host_route(tmp_path):
    """lfvio_host_track_traces over three recordings against lfvio_host_track_trace for each alone, `expand` on: the same files."""
    from lfvio import trace
    from lfvio.host import HostEstimator

    m = Recipe("equirect", (320, 160), (FW, FH))
    cam = er.camera(*m.size)
    srcs = []
    for seed, n in ((0, 12), (1, 12), (2, 9)):
        p = str(tmp_path / f"raw{seed}.lfvt")
        made = trace.make_image_stream(p, seed=seed, n_frames=n, scale=4)
        assert (made["width"], made["height"]) == (FW, FH)
        srcs.append(p)
    small = str(tmp_path / "small.lfvt")
    assert trace.make_image_stream(small, seed=3, n_frames=4, scale=8)["width"] != FW

    def configured(he):
        he.clear_state()
        he.track_config(cam, max_cnt=80, min_dist=12, freq=10, num_samples=100, seed=77)
        he.track_expand(m.cam, m.kind, m.size[0], m.size[1])

    strip = lambda d: {k: v for k, v in d.items() if k != "tracker_ms"}
    want = []
    for k, p in enumerate(srcs):
        he = HostEstimator()  # a fresh estimator and context for every recording
        try:
            configured(he)
            out = str(tmp_path / f"alone{k}.lfvt")
            rc, st = he.track_trace(p, out)
            want.append((rc, strip(st), open(out, "rb").read()))
        finally:
            he.close()
    he = HostEstimator()
    try:
        configured(he)
        outs = [str(tmp_path / f"batch{k}.lfvt") for k in range(3)]
        rc, stats = he.track_traces(srcs, outs)
        got = [(rc, strip(st), open(o, "rb").read()) for st, o in zip(stats, outs)]
        # a fourth recording of another image size: the call fails and writes nothing
        outs4 = [str(tmp_path / f"refused{k}.lfvt") for k in range(4)]
        rc4, _ = he.track_traces(srcs + [small], outs4)
        assert rc4 < 0 and he.track_traces_error() and not any(os.path.exists(o) for o in outs4), (rc4, he.track_traces_error())
    finally:
        he.close()
    assert got == want
    print("host route:", [w[1] for w in want])
    for (rc, st, body), n in zip(want, (12, 12, 9)):
        assert rc == 0 and st["raw_images"] == n and st["published"] >= n - 4 and st["rows"] >= (n - 4) * 20 and len(body) > 0


# ---- 7
def test_host_route_plain(tmp_path):
    """What test_host_route leaves out: `expand` off, the annulus as the base mask, CLAHE on, frames that are tracked only, and a restart.
    Three recordings of 10, 10 and 7 images of 160 x 120 (scale 8; every published message has its 10 rows at this size) at 12.5 Hz, so
    that the FREQ gate lets some frames be tracked without a publication; recording 1's images from the sixth on are stamped 1.5 s later,
    so its gate restarts once.  lfvio_host_track_traces gives, byte for byte and count for count, what lfvio_host_track_trace gives for
    each alone on a fresh estimator; the counts are those of tests/node_ref.Gate over the recording's stamps, which need no device."""
    import struct

    import node_ref as nr
    from lfvio import trace
    from lfvio.host import HostEstimator

    srcs, made, stamps = [], None, []
    for seed, n in ((0, 10), (1, 10), (2, 7)):
        p = str(tmp_path / f"raw{seed}.lfvt")
        made = trace.make_image_stream(p, seed=seed, n_frames=n, scale=8, frame_dt=0.08)
        assert (made["width"], made["height"]) == (160, 120)
        body, at, k, st = bytearray(open(p, "rb").read()), 8, 0, []
        while at < len(body):
            typ, size = struct.unpack_from("<II", body, at)
            if typ == 10:
                t = struct.unpack_from("<d", body, at + 8)[0] + (1.5 if seed == 1 and k >= 5 else 0.0)
                struct.pack_into("<d", body, at + 8, t)
                st.append(t)
                k += 1
            at += 8 + size
        assert k == n
        open(p, "wb").write(body)
        srcs.append(p)
        stamps.append(st)

    # what the node does with these stamps
    counts = []
    for st in stamps:
        g, c = nr.Gate(10), dict(raw_images=float(len(st)), dropped=0.0, restarts=0.0, tracked_only=0.0, published=0.0)
        for t in st:
            a = g.on_stamp(t)
            key = {nr.DROP: "dropped", nr.RESTART: "restarts"}.get(a) or ("published" if g.after_frame() == nr.PUBLISHED else "tracked_only")
            c[key] += 1
        counts.append(c)
    assert [c["restarts"] for c in counts] == [0, 1, 0] and all(c["published"] >= 3 for c in counts)
    assert [c["tracked_only"] for c in counts] == [3, 3, 3] and [c["dropped"] for c in counts] == [1, 2, 1]  # (the skipped first publication and two frames)

    def configured(he):
        he.clear_state()
        he.track_config(made["camera"], max_cnt=40, min_dist=8, freq=10, equalize=True, num_samples=100, seed=77, annulus=made["annulus"])

    strip = lambda d: {k: v for k, v in d.items() if k != "tracker_ms"}
    want = []
    for k, p in enumerate(srcs):
        he = HostEstimator()  # a fresh estimator and context for every recording
        try:
            configured(he)
            out = str(tmp_path / f"alone{k}.lfvt")
            rc, st = he.track_trace(p, out)
            want.append((rc, strip(st), open(out, "rb").read()))
        finally:
            he.close()
    he = HostEstimator()
    try:
        configured(he)
        outs = [str(tmp_path / f"batch{k}.lfvt") for k in range(3)]
        rc, stats = he.track_traces(srcs, outs)
        got = [(rc, strip(st), open(o, "rb").read()) for st, o in zip(stats, outs)]
    finally:
        he.close()
    print("host route, plain:", [w[1] for w in want])
    assert got == want
    for (rc, st, body), c in zip(want, counts):
        assert rc == 0 and {k: st[k] for k in c} == c
        rows, restarts, at = [], 0, 8  # the file's own records: no comparison of empty messages
        while at < len(body):
            typ, size = struct.unpack_from("<II", body, at)
            assert typ != 10
            if typ == 2:
                rows.append(struct.unpack_from("<I", body, at + 16)[0])
                assert size == 12 + 36 * rows[-1]
            restarts += typ == 5
            at += 8 + size
        assert len(rows) == c["published"] and restarts == c["restarts"] and sum(rows) == st["rows"] and min(rows) >= 10, rows
