"""CPU tests of the tracker node's recipe (lf-vio_amd/host/track_node.h), compiled alone with g++ -ffp-contract=off -Wall -Werror behind
a ctypes shim, with no device library on the link line: what FeatureTracker and BatchFeatureTracker share by construction.

  1  FrameBuffers::fill writes the reference's constants — stated here as numbers, not read from the header — for publish 0 and 1, binds
     the seven arrays, and draws 8 * num_samples words of the stream's generator in row order exactly when publish is set
  2  seedSamples with a nonzero seed is std::mt19937(seed), whose raw outputs tests/node_ref.py restates as
     np.random.RandomState(seed).randint(0, 2**32, dtype=uint32); seed 0 gives two different generators
  3  the base mask: the annulus equals lfvio.engine.annulus_mask at 16 x 12 and 33 x 17 with a centre off the pixel grid; a given mask is
     handed on as it is; neither: {0, 0, null}
  4  NodeSettings::apply against a route that records its calls: expand off and on, a later change of the step only and of the source's
     size only, and a third call that fails — it stops there, returns that status and repeats the whole first-use block on the next image
  5  the check of one image's arguments, the mapping of the gate's answer to a Result, the feature message's rows"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <string>

#include "track_node.h"
using namespace lfvio;

// FeatureTracker::DROPPED and the others are TrackResults', at the values the C ABI's callers know
static_assert(TrackResults::DROPPED == 0 && TrackResults::RESTART == 1 && TrackResults::TRACKED_ONLY == 2 && TrackResults::FIRST_PUBLICATION_SKIPPED == 3 &&
                  TrackResults::PUBLISHED == 4,
              "the results' values");

static TrackerConfig config(int max_cnt, int min_dist, int num_samples) {
  TrackerConfig c;
  c.max_cnt = max_cnt, c.min_dist = min_dist, c.num_samples = num_samples;
  return c;
}

// iv[24], dv[4], words[8 * num_samples] (0xEEEEEEEE where nothing was drawn), next[2] = the generator's next output behind fill and
// that of a twin seeded alike that never saw fill
extern "C" void tn_fill(int publish, unsigned seed, int num_samples, int max_cnt, int min_dist, int tw, int th, double stamp, int *iv, double *dv,
                        unsigned *words, unsigned *next) {
  static const unsigned char pixel = 0;
  const TrackerConfig c = config(max_cnt, min_dist, num_samples);
  std::mt19937 rng, twin;
  seedSamples(rng, seed), seedSamples(twin, seed);
  FrameBuffers b;
  LfvioTrackFrameIn in;
  LfvioTrackFrameOut out;
  LfvioTrackMessage msg;
  std::memset(&in, 0xEE, sizeof in), std::memset(&out, 0xEE, sizeof out), std::memset(&msg, 0xEE, sizeof msg);
  b.fill(c, tw, th, &pixel, stamp, publish != 0, rng, &in, &out, &msg);
  const int i[24] = {in.width, in.height, in.publish, in.win_size, in.max_level, in.max_iterations, in.border, in.max_count, in.min_distance, in.mask_radius,
                     in.num_samples, in.capacity, in.sample_words == nullptr, in.sample_words == b.words.data(), in.image == &pixel, in.camera == &c.camera,
                     out.pts == b.pts.data() && b.pts.size() == 2u * LFVIO_TRACK_MAX_POINTS, out.ids == b.ids.data() && b.ids.size() == 1u * LFVIO_TRACK_MAX_POINTS,
                     out.track_cnt == b.track_cnt.data() && b.track_cnt.size() == 1u * LFVIO_TRACK_MAX_POINTS,
                     out.un_pts == b.un_pts.data() && b.un_pts.size() == 2u * LFVIO_TRACK_MAX_POINTS,
                     out.un_pts_3d == b.un_pts_3d.data() && b.un_pts_3d.size() == 3u * LFVIO_TRACK_MAX_POINTS,
                     out.velocity_3d == b.velocity_3d.data() && b.velocity_3d.size() == 3u * LFVIO_TRACK_MAX_POINTS,
                     msg.rows == b.rows.data() && b.rows.size() == 9u * LFVIO_TRACK_MAX_POINTS, msg.num_rows + 100 * out.num_points};
  std::memcpy(iv, i, sizeof i);
  dv[0] = in.time, dv[1] = in.epsilon, dv[2] = in.min_eig_threshold, dv[3] = in.quality_level;
  for (size_t k = 0; k < (size_t)num_samples * 8; k++) words[k] = k < b.words.size() ? b.words[k] : 0xEEEEEEEEu;
  next[0] = (unsigned)rng(), next[1] = (unsigned)twin();
}

extern "C" void tn_seed(unsigned seed, int n, unsigned *out) {
  std::mt19937 rng;
  seedSamples(rng, seed);
  for (int k = 0; k < n; k++) out[k] = (unsigned)rng();
}

// kind 0: none, 1: annulus, 2: given (gw x gh).  out[3] = {width, height, where the pixels are: 0 null, 1 the storage, 2 the config's}
extern "C" void tn_mask(int kind, int tw, int th, double cx, double cy, double max_r, double min_r, int gw, int gh, const unsigned char *given, int *out,
                        unsigned char *pixels) {
  TrackerConfig c;
  if (kind == 1) c.annulus = true, c.center_x = cx, c.center_y = cy, c.max_r = max_r, c.min_r = min_r;
  if (kind == 2) c.mask.assign(given, given + (size_t)gw * gh), c.mask_width = gw, c.mask_height = gh, c.annulus = true;  // a given mask wins
  std::vector<unsigned char> storage;
  const BaseMask m = baseMask(c, tw, th, &storage);
  out[0] = m.width, out[1] = m.height, out[2] = !m.pixels ? 0 : m.pixels == storage.data() ? 1 : m.pixels == c.mask.data() ? 2 : -1;
  if (m.pixels) std::memcpy(pixels, m.pixels, (size_t)m.width * m.height);
}

// the route that records: one line per call into `log`; call number `fail_at` (from 1) returns `fail_rc`
struct Recorder final : SettingsRoute {
  std::string log;
  int calls = 0, fail_at = 0, fail_rc = 0;
  int done(const std::string &line) {
    log += line + "\n";
    return ++calls == fail_at ? fail_rc : 0;
  }
  int mask(int w, int h, const unsigned char *p) override {
    long sum = 0;
    for (long k = 0; p && k < (long)w * h; k++) sum += p[k];
    return done("mask " + std::to_string(w) + " " + std::to_string(h) + " " + (p ? std::to_string(sum) : std::string("null")));
  }
  int clahe(const LfvioClaheIn *c) override {
    return done(c ? "clahe " + std::to_string(c->clip_limit) + " " + std::to_string(c->tiles_x) + " " + std::to_string(c->tiles_y) : std::string("clahe null"));
  }
  int format(const LfvioImageFormat *f) override { return done("format " + std::to_string(f->encoding) + " " + std::to_string(f->step)); }
  int map(const LfvioRemapIn *in) override {
    return done("map " + std::to_string(in->kind) + " " + std::to_string(in->width) + " " + std::to_string(in->height) + " " + std::to_string(in->M[4]) + " " +
                std::to_string(in->proj->camera->cx) + " " + std::to_string(in->proj->inv_poly[2]));
  }
  int source(const LfvioTrackSource *s) override {
    return done(s ? "source " + std::to_string(s->src_width) + " " + std::to_string(s->src_height) : std::string("source null"));
  }
};

struct Node {
  TrackerConfig cfg;
  NodeSettings settings;
};
extern "C" void *tn_node(int expand, int equalize, int annulus) {
  Node *n = new Node();
  n->cfg.equalize = equalize != 0;
  if (annulus) n->cfg.annulus = true, n->cfg.center_x = 8.0, n->cfg.center_y = 6.0, n->cfg.max_r = 5.0, n->cfg.min_r = 2.0;
  if (expand) {
    TrackerConfig::Expand &x = n->cfg.expand;
    x.on = true, x.kind = LFVIO_MAP_PERSPECTIVE, x.width = 20, x.height = 10, x.M[4] = 0.5, x.src_camera.cx = 31.25, x.inv_poly[2] = 7.5;
  }
  return n;
}
extern "C" void tn_node_delete(void *n) { delete (Node *)n; }
// one image: -> the status; log[cap] the calls made; state[5] = ready_, format_, source_
extern "C" int tn_apply(void *h, int width, int height, int encoding, int step, int fail_at, int fail_rc, char *log, int cap, int *state) {
  Node *n = (Node *)h;
  Recorder r;
  r.fail_at = fail_at, r.fail_rc = fail_rc;
  const int rc = n->settings.apply(n->cfg, width, height, {encoding, step}, r);
  std::snprintf(log, (size_t)cap, "%s", r.log.c_str());
  const NodeSettings &s = n->settings;
  state[0] = s.ready_, state[1] = s.format_.encoding, state[2] = s.format_.step, state[3] = s.source_.src_width, state[4] = s.source_.src_height;
  return rc;
}

extern "C" int tn_args_bad(int width, int height, int step, int encoding, int null_pixels) {
  static const unsigned char pixel = 0;
  return imageArgsBad(width, height, step, encoding, null_pixels ? nullptr : &pixel);
}
extern "C" int tn_result(int after) { return frameResult((ImageGate::Frame)after); }
extern "C" int tn_message(double stamp, int num_rows, double *t, float *v) {
  FrameBuffers b;
  for (size_t k = 0; k < b.rows.size(); k++) b.rows[k] = (float)k + 0.5f;
  TraceImage msg;
  msg.t = -1.0, msg.v.assign(5, 9.0f);
  b.message(stamp, num_rows, &msg);
  *t = msg.t;
  for (size_t k = 0; k < msg.v.size(); k++) v[k] = msg.v[k];
  return (int)msg.size();
}
'''
u32p, i32p, f64p = C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_double)


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="track_node_")
    src, so = os.path.join(d, "node.cpp"), os.path.join(d, "libnode.so")
    open(src, "w").write(SRC)
    # no -l at all: the header names no device symbol, and -z defs makes the link fail if it did
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-Wl,-z,defs", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "host"), src, "-o", so])
    so = C.CDLL(so)
    so.tn_fill.argtypes = [C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, i32p, f64p, u32p, u32p]
    so.tn_seed.argtypes = [C.c_uint, C.c_int, u32p]
    so.tn_mask.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, i32p, C.c_void_p]
    so.tn_node.restype = C.c_void_p
    so.tn_node_delete.argtypes = [C.c_void_p]
    so.tn_apply.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, i32p]
    so.tn_message.argtypes = [C.c_double, C.c_int, f64p, C.POINTER(C.c_float)]
    return so


def mt19937(seed, n):
    """The raw outputs of std::mt19937(seed), as tests/node_ref.ImageNode draws them."""
    return np.random.RandomState(seed).randint(0, 2 ** 32, size=n, dtype=np.uint32)


# ---- 1
@pytest.mark.parametrize("publish", [0, 1])
def test_fill(lib, publish):
    seed, S, max_cnt, min_dist, tw, th, stamp = 77, 5, 40, 8, 33, 17, 1403636579.76
    iv, dv, words, nxt = np.zeros(24, np.int32), np.zeros(4), np.zeros(8 * S, np.uint32), np.zeros(2, np.uint32)
    lib.tn_fill(publish, seed, S, max_cnt, min_dist, tw, th, stamp, _p(iv, i32p), _p(dv, f64p), _p(words, u32p), _p(nxt, u32p))
    want = dict(width=tw, height=th, publish=publish,
                win_size=41, max_level=3,          # cv::calcOpticalFlowPyrLK(..., cv::Size(41, 41), 3), feature_tracker.cpp:127
                max_iterations=30, border=1,       # ... its default criteria (COUNT + EPS, 30, 0.01); BORDER_SIZE of inBorder, :5-10
                max_count=max_cnt,                 # MAX_CNT - forw_pts.size(), :166
                min_distance=min_dist,             # goodFeaturesToTrack(..., 0.01, MIN_DIST, mask), :166
                mask_radius=min_dist,              # cv::circle(mask, it.second.first, MIN_DIST, 0, -1), :80
                num_samples=S, capacity=4096)
    assert dict(zip(want, iv[:12].tolist())) == want
    assert dv.tolist() == [stamp, 0.01, 1e-4, 0.01]  # the time; epsilon and minEigThreshold of :127's defaults; qualityLevel of :166
    assert iv[14:23].tolist() == [1] * 9  # the image, the camera of the config, the seven arrays at their sizes
    assert iv[23] == 0  # num_rows = 0 and a zeroed out
    stream = mt19937(seed, 8 * S + 1)
    if publish:
        assert (iv[12], iv[13]) == (0, 1)
        assert np.array_equal(words, stream[:-1])  # S rows of 8, in row order
        assert nxt[0] == stream[-1] and nxt[1] == stream[0]  # exactly 8 * S were drawn
    else:
        assert iv[12] == 1  # sample_words is null
        assert np.all(words == 0xEEEEEEEE)
        assert nxt[0] == nxt[1] == stream[0]  # the generator's next output is unchanged


def test_fill_draws_for_the_count_asked(lib):
    for S in (1, 100):
        iv, dv, words, nxt = np.zeros(24, np.int32), np.zeros(4), np.zeros(8 * S, np.uint32), np.zeros(2, np.uint32)
        lib.tn_fill(1, 5, S, 150, 30, 16, 16, 0.0, _p(iv, i32p), _p(dv, f64p), _p(words, u32p), _p(nxt, u32p))
        stream = mt19937(5, 8 * S + 1)
        assert iv[10] == S and np.array_equal(words, stream[:-1]) and nxt[0] == stream[-1]


# ---- 2
def test_seeding(lib):
    for seed in (1, 77, 2 ** 32 - 1):
        got = np.zeros(64, np.uint32)
        lib.tn_seed(seed, 64, _p(got, u32p))
        assert np.array_equal(got, mt19937(seed, 64)), seed
    got = np.zeros(4, np.uint32)
    lib.tn_seed(1, 4, _p(got, u32p))
    assert got.tolist() == [1791095845, 4282876139, 3093770124, 4005303368]  # std::mt19937(1)
    a, b = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    lib.tn_seed(0, 16, _p(a, u32p)), lib.tn_seed(0, 16, _p(b, u32p))
    assert not np.array_equal(a, b) and not np.array_equal(a, mt19937(0, 16))  # 0: std::random_device, not the seed 0


# ---- 3
@pytest.mark.parametrize("w,h,an", [(16, 12, (7.3, 5.6, 5.2, 1.9)), (33, 17, (16.45, 8.2, 9.75, 3.1)), (33, 17, (16.0, 8.0, 5.0, 2.0))])
def test_annulus(lib, w, h, an):
    from lfvio.engine import annulus_mask

    out, px = np.zeros(3, np.int32), np.full(w * h, 7, np.uint8)
    lib.tn_mask(1, w, h, *an, 0, 0, None, _p(out, i32p), px.ctypes.data)
    want = annulus_mask(w, h, *an)
    assert out.tolist() == [w, h, 1] and np.array_equal(px.reshape(h, w), want)
    assert 0 < (want == 255).sum() < w * h and want[int(round(an[1])), int(round(an[0]))] == 0  # a ring: the hole and the outside are there


def test_given_mask_and_none(lib):
    out, px = np.zeros(3, np.int32), np.zeros(64, np.uint8)
    lib.tn_mask(0, 16, 12, 0, 0, 0, 0, 0, 0, None, _p(out, i32p), px.ctypes.data)
    assert out.tolist() == [0, 0, 0]
    given = np.random.default_rng(3).integers(0, 2, (5, 9)).astype(np.uint8) * 255
    lib.tn_mask(2, 16, 12, 8.0, 6.0, 5.0, 2.0, 9, 5, given.ctypes.data, _p(out, i32p), px.ctypes.data)
    assert out.tolist() == [9, 5, 2] and np.array_equal(px[:45].reshape(5, 9), given)  # its own size, its own pixels, nothing rasterised


# ---- 4
W, H = 64, 48
MONO8, BGR8 = 0, 2


class Node:
    def __init__(self, lib, expand=0, equalize=0, annulus=0):
        self.lib, self.h = lib, lib.tn_node(expand, equalize, annulus)

    def __call__(self, width, height, encoding, step, fail_at=0, fail_rc=0):
        log, state = C.create_string_buffer(1024), np.zeros(5, np.int32)
        rc = self.lib.tn_apply(self.h, width, height, encoding, step, fail_at, fail_rc, log, 1024, _p(state, i32p))
        return rc, log.value.decode().splitlines(), state.tolist()

    def close(self):
        self.lib.tn_node_delete(self.h)


@pytest.fixture
def node(lib):
    made = []

    def make(**kw):
        made.append(Node(lib, **kw))
        return made[-1]
    yield make
    for n in made:
        n.close()


RING = str(255 * int(((lambda d2: (d2 <= 25.0) & (d2 > 4.0))((np.mgrid[0:H, 0:W][1] - 8.0) ** 2 + (np.mgrid[0:H, 0:W][0] - 6.0) ** 2)).sum()))
FIRST_OFF = [f"mask {W} {H} {RING}", "clahe 3.000000 8 8", f"format {BGR8} {3 * W + 1}", "source null"]


def test_settings_expand_off(node):
    n = node(equalize=1, annulus=1)
    assert n(W, H, BGR8, 3 * W + 1) == (0, FIRST_OFF, [1, BGR8, 3 * W + 1, W, H])
    assert n(W, H, BGR8, 3 * W + 1) == (0, [], [1, BGR8, 3 * W + 1, W, H])  # a steady stream sets nothing again
    # without expand the source's size is nobody's business: a later size changes nothing
    assert n(W + 2, H, BGR8, 3 * W + 1)[:2] == (0, [])
    plain = node()
    assert plain(W, H, MONO8, W)[:2] == (0, ["mask 0 0 null", "clahe null", f"format {MONO8} {W}", "source null"])


def test_settings_expand_on(node):
    n = node(expand=1, annulus=1)
    ring = str(255 * int(((lambda d2: (d2 <= 25.0) & (d2 > 4.0))((np.mgrid[0:10, 0:20][1] - 8.0) ** 2 + (np.mgrid[0:10, 0:20][0] - 6.0) ** 2)).sum()))
    first = [f"mask 20 10 {ring}", "clahe null", f"format {MONO8} {W}", "map 1 20 10 0.500000 31.250000 7.500000", f"source {W} {H}"]  # the mask has the TRACKED size
    assert n(W, H, MONO8, W) == (0, first, [1, MONO8, W, W, H])
    assert n(W, H, MONO8, W)[:2] == (0, [])


def test_settings_later_changes(node):
    n = node(expand=1)
    assert n(W, H, MONO8, W)[0] == 0
    assert n(W, H, MONO8, W + 4) == (0, [f"format {MONO8} {W + 4}"], [1, MONO8, W + 4, W, H])  # the step only
    assert n(W, H, BGR8, W + 4)[1] == [f"format {BGR8} {W + 4}"]  # (W + 4 is no bgr8 step of W pixels: judging it is imageArgsBad's)
    assert n(W + 16, H, BGR8, W + 4) == (0, [f"source {W + 16} {H}"], [1, BGR8, W + 4, W + 16, H])  # the source's size only
    assert n(W + 16, H + 2, MONO8, W + 16) == (0, [f"source {W + 16} {H + 2}", f"format {MONO8} {W + 16}"], [1, MONO8, W + 16, W + 16, H + 2])  # both: in this order
    # a later change that fails keeps what was set, and is tried again
    assert n(W, H + 2, MONO8, W + 16, fail_at=1, fail_rc=-5) == (-5, [f"source {W} {H + 2}"], [1, MONO8, W + 16, W + 16, H + 2])
    assert n(W, H + 2, MONO8, W + 16) == (0, [f"source {W} {H + 2}"], [1, MONO8, W + 16, W, H + 2])


@pytest.mark.parametrize("expand", [0, 1])
def test_settings_failing_third_call(node, expand):
    n = node(expand=expand, equalize=1)
    tail = ["map 1 20 10 0.500000 31.250000 7.500000", f"source {W} {H}"] if expand else ["source null"]
    first = ["mask 0 0 null", "clahe 3.000000 8 8", f"format {MONO8} {W}"] + tail
    assert n(W, H, MONO8, W, fail_at=3, fail_rc=-7) == (-7, first[:3], [0, MONO8, 0, 0, 0])  # stops there; not ready, nothing remembered
    assert n(W, H, MONO8, W + 1) == (0, first[:2] + [f"format {MONO8} {W + 1}"] + tail, [1, MONO8, W + 1, W, H])  # the whole block again
    for at in range(1, len(first) + 1):  # every place of the first-use block
        m = node(expand=expand, equalize=1)
        assert m(W, H, MONO8, W, fail_at=at, fail_rc=-2) == (-2, first[:at], [0, MONO8, 0, 0, 0]), at


# ---- 5
def test_image_args(lib):
    assert lib.tn_args_bad(64, 48, 64, MONO8, 0) == 0 and lib.tn_args_bad(64, 48, 192, BGR8, 0) == 0 and lib.tn_args_bad(64, 48, 70, MONO8, 0) == 0
    assert lib.tn_args_bad(64, 48, 64, MONO8, 1)  # null pixels
    assert lib.tn_args_bad(0, 48, 64, MONO8, 0) and lib.tn_args_bad(64, 0, 64, MONO8, 0) and lib.tn_args_bad(64, 48, 0, MONO8, 0)
    assert lib.tn_args_bad(64, 48, 63, MONO8, 0) and lib.tn_args_bad(64, 48, 191, BGR8, 0)  # step < width * bytes per pixel
    assert lib.tn_args_bad(64, 48, 64, 1, 0) and lib.tn_args_bad(64, 48, 640, 8, 0)  # codes outside the table


def test_results_and_message(lib):
    import node_ref as nr

    assert [lib.tn_result(a) for a in (nr.TRACKED, nr.FIRST_PUBLICATION, nr.PUBLISHED)] == [2, 3, 4]
    t, v = C.c_double(), np.zeros(64, np.float32)
    assert lib.tn_message(12.5, 3, C.byref(t), _p(v, C.POINTER(C.c_float))) == 3
    assert t.value == 12.5 and np.array_equal(v[:27], np.arange(27, dtype=np.float32) + 0.5)
    assert lib.tn_message(1.0, 0, C.byref(t), _p(v, C.POINTER(C.c_float))) == 0  # a message without rows replaces what was there
