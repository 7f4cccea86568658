// batch_tracker.cpp — see batch_tracker.h.  Every statement that decides what a stream publishes is FeatureTracker::onImage's
// (feature_tracker.cpp), per stream.
#include "batch_tracker.h"

#include "../csrc/image_format.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

namespace lfvio {

BatchFeatureTracker::BatchFeatureTracker(const TrackerConfig &config, int streams, lfvio_ctx *ctx, int device) : cfg_(config), ctx_(ctx) {
  if (streams < 1 || streams > LFVIO_TRACK_BATCH_MAX_SLOTS) {
    status = LFVIO_ERR_ARG;
    error_ = "BatchFeatureTracker: streams outside [1, 64]";
    ctx_ = nullptr;
    return;
  }
  if (!ctx_) {
    ctx_ = lfvio_create(device);
    own_ = ctx_ != nullptr;
  }
  if (!ctx_) {
    status = LFVIO_ERR_DEVICE;  // there is no host fallback: every onRound returns it
    error_ = "lfvio_create failed";
    return;
  }
  status = lfvio_track_batch_reserve(ctx_, streams);
  if (status != LFVIO_OK) {  // every onRound returns it
    error_ = std::string("lfvio_track_batch_reserve: ") + lfvio_last_error(ctx_);
    failed_ = true;
    return;
  }
  gate.resize((size_t)streams);
  for (ImageGate &g : gate) g.freq = cfg_.freq;
  rng_.resize((size_t)streams);
  for (std::mt19937 &r : rng_) {
    if (cfg_.ransac_seed != 0) {
      r.seed(cfg_.ransac_seed);
    } else {  // as FeatureTracker
      std::random_device rd;
      std::vector<std::uint_least32_t> v(10);
      std::generate(v.begin(), v.end(), std::ref(rd));
      std::seed_seq seq(v.begin(), v.end());
      r.seed(seq);
    }
  }
  const size_t cap = LFVIO_TRACK_MAX_POINTS;
  words_.resize((size_t)streams), arrays_.resize((size_t)streams);
  in_.resize((size_t)streams), out_.resize((size_t)streams), msg_.resize((size_t)streams);
  for (Arrays &a : arrays_) {
    a.pts.resize(cap * 2), a.un_pts.resize(cap * 2), a.un_pts_3d.resize(cap * 3), a.velocity_3d.resize(cap * 3), a.rows.resize(cap * 9);
    a.ids.resize(cap), a.track_cnt.resize(cap);
  }
}

BatchFeatureTracker::~BatchFeatureTracker() {
  if (ctx_) {  // the context may be the caller's: the batch's settings go back to those of a fresh context, its memory is freed
    (void)lfvio_track_batch_source(ctx_, nullptr);
    (void)lfvio_track_batch_format(ctx_, nullptr);
    (void)lfvio_track_batch_clahe(ctx_, nullptr);
    (void)lfvio_track_batch_reserve(ctx_, 0);
  }
  if (own_) lfvio_destroy(ctx_);
}

const char *BatchFeatureTracker::error() const { return ctx_ && error_.empty() ? lfvio_last_error(ctx_) : error_.c_str(); }

// the base mask, EQUALIZE, the format, the maps and the source, once (FeatureTracker::onImage's `ready_` block, for every slot)
int BatchFeatureTracker::setup(int tw, int th, const LfvioImageFormat &format, const LfvioTrackSource &source) {
  const TrackerConfig::Expand &ex = cfg_.expand;
  int rc = LFVIO_OK;
  if (!cfg_.mask.empty()) {
    rc = lfvio_track_batch_set_mask(ctx_, -1, cfg_.mask_width, cfg_.mask_height, cfg_.mask.data());
  } else if (cfg_.annulus) {
    std::vector<unsigned char> m((size_t)tw * th);
    const double hi = cfg_.max_r * cfg_.max_r, lo = cfg_.min_r * cfg_.min_r;
    for (int y = 0; y < th; y++)
      for (int x = 0; x < tw; x++) {
        const double dx = x - cfg_.center_x, dy = y - cfg_.center_y, d2 = dx * dx + dy * dy;
        m[(size_t)y * tw + x] = d2 <= hi && d2 > lo ? 255 : 0;
      }
    rc = lfvio_track_batch_set_mask(ctx_, -1, tw, th, m.data());
  } else {
    rc = lfvio_track_batch_set_mask(ctx_, -1, 0, 0, nullptr);
  }
  if (rc == LFVIO_OK) {
    const LfvioClaheIn clahe = {3.0, 8, 8};
    rc = lfvio_track_batch_clahe(ctx_, cfg_.equalize ? &clahe : nullptr);
  }
  if (rc == LFVIO_OK) rc = lfvio_track_batch_format(ctx_, &format);
  if (rc == LFVIO_OK && ex.on) {  // the map of the expanded image through the source camera in every slot: one launch
    LfvioProjector proj = {};
    proj.camera = &ex.src_camera;
    std::memcpy(proj.inv_poly, ex.inv_poly, sizeof proj.inv_poly);
    LfvioRemapIn rin = {};
    rin.proj = &proj, rin.kind = ex.kind, rin.width = ex.width, rin.height = ex.height;
    std::memcpy(rin.M, ex.M, sizeof rin.M);
    rc = lfvio_track_batch_map(ctx_, -1, &rin);
  }
  if (rc == LFVIO_OK) rc = lfvio_track_batch_source(ctx_, ex.on ? &source : nullptr);
  if (rc != LFVIO_OK) return rc;
  format_ = format, source_ = source, ready_ = true;
  return LFVIO_OK;
}

int BatchFeatureTracker::onRound(BatchEntry *entries) {
  if (!ctx_ || failed_) return status;  // the constructor failed: error() says how
  const int n = streams();
  error_.clear(), disagreed = false;
  // every entry's arguments first: a round is refused as a whole
  for (int i = 0; i < n; i++) {
    const BatchEntry &e = entries[i];
    if (!e.present) continue;
    const LfvioImageFormat format = {e.encoding, e.step};
    if (!e.pixels || e.width < 1 || e.height < 1 || e.step < 1 || imgfmt_check(format, e.width, e.height)) {
      error_ = "BatchFeatureTracker::onRound: null pixels, an unknown encoding, or step < width * bytes per pixel";
      return status = LFVIO_ERR_ARG;
    }
  }
  // the images that would reach the tracker must agree.  The gates move only behind this check, so it is made on their copies.
  int first = -1;
  {
    std::vector<ImageGate> trial = gate;
    for (int i = 0; i < n; i++) {
      const BatchEntry &e = entries[i];
      if (!e.present || trial[i].onStamp(e.stamp) != ImageGate::TRACK) continue;
      if (first < 0) {
        first = i;
        continue;
      }
      const BatchEntry &f = entries[first];
      if (e.width != f.width || e.height != f.height || e.step != f.step || e.encoding != f.encoding) {
        error_ = "BatchFeatureTracker::onRound: the images of a round disagree in width, height, step or encoding";
        disagreed = true;
        return status = LFVIO_ERR_ARG;
      }
    }
  }
  std::vector<char> active((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    BatchEntry &e = entries[i];
    if (!e.present) continue;
    const ImageGate::Stamp what = gate[i].onStamp(e.stamp);  // feature_tracker_node.cpp:30-62
    if (what == ImageGate::DROP) e.result = FeatureTracker::DROPPED;
    else if (what == ImageGate::RESTART) e.result = FeatureTracker::RESTART;
    else active[i] = 1;
  }
  if (first < 0) return LFVIO_OK;  // nothing reaches the tracker
  const BatchEntry &f = entries[first];
  const TrackerConfig::Expand &ex = cfg_.expand;
  const int tw = ex.on ? ex.width : f.width, th = ex.on ? ex.height : f.height;
  const LfvioImageFormat format = {f.encoding, f.step};
  const LfvioTrackSource source = {f.width, f.height};
  if (!ready_)
    if (int rc = setup(tw, th, format, source)) return status = rc;
  if (ex.on && (source.src_width != source_.src_width || source.src_height != source_.src_height)) {  // a driver that changes its size
    if (int rc = lfvio_track_batch_source(ctx_, &source)) return status = rc;
    source_ = source;
  }
  if (format.encoding != format_.encoding || format.step != format_.step) {  // a driver that changes its rows
    if (int rc = lfvio_track_batch_format(ctx_, &format)) return status = rc;
    format_ = format;
  }
  const int S = cfg_.num_samples;
  for (int i = 0; i < n; i++) {
    LfvioTrackFrameIn &in = in_[i];
    in = LfvioTrackFrameIn();
    if (!active[i]) continue;  // image null: the slot is idle in this call
    const BatchEntry &e = entries[i];
    const bool pub = gate[i].publish;
    if (pub) {  // num_samples x 8 raw outputs of the stream's generator; nothing is drawn for a frame that is only tracked
      words_[i].resize((size_t)std::max(S, 0) * 8);
      for (unsigned &w : words_[i]) w = (unsigned)rng_[i]();
    }
    in.width = tw, in.height = th, in.image = e.pixels, in.time = e.stamp, in.publish = pub ? 1 : 0, in.camera = &cfg_.camera;
    in.win_size = 41, in.max_level = 3, in.max_iterations = 30, in.epsilon = 0.01, in.min_eig_threshold = 1e-4, in.border = 1;
    in.max_count = cfg_.max_cnt, in.quality_level = 0.01, in.min_distance = cfg_.min_dist, in.mask_radius = cfg_.min_dist;
    in.num_samples = S, in.sample_words = pub ? words_[i].data() : nullptr, in.capacity = LFVIO_TRACK_MAX_POINTS;
    Arrays &a = arrays_[i];
    LfvioTrackFrameOut &out = out_[i];
    out = LfvioTrackFrameOut();
    out.pts = a.pts.data(), out.ids = a.ids.data(), out.track_cnt = a.track_cnt.data();
    out.un_pts = a.un_pts.data(), out.un_pts_3d = a.un_pts_3d.data(), out.velocity_3d = a.velocity_3d.data();
    msg_[i].num_rows = 0, msg_[i].rows = a.rows.data();
  }
  if (int rc = lfvio_track_batch_frame(ctx_, n, in_.data(), out_.data(), msg_.data())) return status = rc;
  for (int i = 0; i < n; i++) {
    if (!active[i]) continue;
    BatchEntry &e = entries[i];
    const ImageGate::Frame after = gate[i].afterFrame();  // :113-178
    if (after == ImageGate::TRACKED_ONLY) e.result = FeatureTracker::TRACKED_ONLY;
    else if (after == ImageGate::FIRST_PUBLICATION) e.result = FeatureTracker::FIRST_PUBLICATION_SKIPPED;
    else {
      e.result = FeatureTracker::PUBLISHED;
      e.msg.t = e.stamp;
      e.msg.v.assign(arrays_[i].rows.begin(), arrays_[i].rows.begin() + (size_t)msg_[i].num_rows * 9);
    }
  }
  return LFVIO_OK;
}

namespace {
void put(std::vector<char> *out, const void *p, size_t n) {
  const char *c = (const char *)p;
  out->insert(out->end(), c, c + n);
}
void record(std::vector<char> *out, uint32_t type, const void *a, size_t na, const void *b = nullptr, size_t nb = 0) {
  const uint32_t head[2] = {type, (uint32_t)(na + nb)};
  put(out, head, sizeof head);
  put(out, a, na);
  if (nb) put(out, b, nb);
}
// One recording being read: every record in front of the next raw image is copied to `out`, the image waits in `buf`
struct Cursor {
  std::FILE *f = nullptr;
  std::vector<char> buf;
  bool pending = false, bad = false;
  ~Cursor() {
    if (f) std::fclose(f);
  }
  void advance(std::vector<char> *out) {
    pending = false;
    for (;;) {
      uint32_t head[2];
      if (std::fread(head, 4, 2, f) != 2) return;
      buf.resize(head[1]);
      if (head[1] && std::fread(buf.data(), 1, head[1], f) != head[1]) {
        bad = true;
        return;
      }
      if (head[0] == 10) {
        pending = true;
        return;
      }
      record(out, head[0], buf.data(), buf.size());
    }
  }
};
}  // namespace

int trackRecordings(BatchFeatureTracker &tracker, int n, const char *const *in_paths, std::vector<std::vector<char>> *outs, TrackStats *stats) {
  std::vector<TrackStats> st((size_t)n);
  if (n > 0) std::memset(st.data(), 0, (size_t)n * sizeof(TrackStats));
  auto finish = [&](int rc) {
    if (stats)
      for (int i = 0; i < n; i++) stats[i] = st[i];
    return rc;
  };
  if (tracker.status != LFVIO_OK) return finish(-2);  // the tracker's constructor failed
  if (n < 1 || n != tracker.streams()) return finish(-3);
  outs->assign((size_t)n, std::vector<char>());
  std::vector<Cursor> cur((size_t)n);
  for (int i = 0; i < n; i++) {
    {
      Trace check;  // every refusal of the loader is this call's: the pass below trusts the lengths
      if (!check.load(in_paths[i])) return finish(-3);
    }
    cur[i].f = std::fopen(in_paths[i], "rb");
    char file_head[8];
    if (!cur[i].f || std::fread(file_head, 1, 8, cur[i].f) != 8) return finish(-3);
    put(&(*outs)[i], file_head, 8);
    cur[i].advance(&(*outs)[i]);
    if (cur[i].bad) return finish(-3);
  }
  std::vector<BatchEntry> entries((size_t)n);
  for (;;) {
    bool any = false;
    for (int i = 0; i < n; i++) {
      BatchEntry &e = entries[i];
      e.present = cur[i].pending;
      if (!e.present) continue;
      any = true;
      uint32_t dims[4];  // width, height, step, encoding
      std::memcpy(&e.stamp, cur[i].buf.data(), 8), std::memcpy(dims, cur[i].buf.data() + 8, 16);
      e.width = (int)dims[0], e.height = (int)dims[1], e.step = (int)dims[2], e.encoding = (int)dims[3];
      e.pixels = (const unsigned char *)cur[i].buf.data() + 24;
      st[i].raw_images++;
    }
    if (!any) break;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = tracker.onRound(entries.data());
    const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    if (rc < 0) return finish(tracker.disagreed ? -4 : -2);  // no silent continuation
    for (int i = 0; i < n; i++) {
      BatchEntry &e = entries[i];
      if (!e.present) continue;
      st[i].tracker_ms += ms;  // the round's: the streams share the call
      std::vector<char> *out = &(*outs)[i];
      switch (e.result) {
        case FeatureTracker::DROPPED:
          st[i].dropped++;
          break;
        case FeatureTracker::RESTART:  // std_msgs/Bool(true) on the restart topic (feature_tracker_node.cpp:44-46)
          st[i].restarts++;
          record(out, 5, &e.stamp, 8);
          break;
        case FeatureTracker::PUBLISHED: {
          st[i].published++, st[i].rows += (double)e.msg.size();
          struct {
            double t;
            uint32_t n;
          } __attribute__((packed)) mh = {e.msg.t, (uint32_t)e.msg.size()};
          static_assert(sizeof mh == 12, "packed");
          record(out, 2, &mh, sizeof mh, e.msg.v.data(), e.msg.v.size() * sizeof(float));
          break;
        }
        default:  // tracked only, or the first publication, which the node skips
          st[i].tracked_only++;
      }
      cur[i].advance(out);
      if (cur[i].bad) return finish(-3);
    }
  }
  return finish(0);
}

}  // namespace lfvio
