// batch_tracker.cpp — see batch_tracker.h.  Every statement that decides what a stream publishes is track_node.h's, as it is for
// FeatureTracker (feature_tracker.cpp); this file holds the batch's device calls and what is the batch's own.  The walk over the
// recordings is trace_rewrite.cpp's.
#include "batch_tracker.h"

namespace lfvio {

namespace {
struct BatchRoute final : SettingsRoute {  // the settings of every slot of the context's batch
  lfvio_ctx *ctx;
  explicit BatchRoute(lfvio_ctx *c) : ctx(c) {}
  int mask(int width, int height, const unsigned char *pixels) override { return lfvio_track_batch_set_mask(ctx, -1, width, height, pixels); }
  int clahe(const LfvioClaheIn *clahe) override { return lfvio_track_batch_clahe(ctx, clahe); }
  int format(const LfvioImageFormat *format) override { return lfvio_track_batch_format(ctx, format); }
  int map(const LfvioRemapIn *in) override { return lfvio_track_batch_map(ctx, -1, in); }  // one launch
  int source(const LfvioTrackSource *source) override { return lfvio_track_batch_source(ctx, source); }
};
}  // namespace

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
  for (std::mt19937 &r : rng_) seedSamples(r, cfg_.ransac_seed);
  buffers_.resize((size_t)streams);
  in_.resize((size_t)streams), out_.resize((size_t)streams), msg_.resize((size_t)streams);
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

int BatchFeatureTracker::onRound(BatchEntry *entries) {
  if (!ctx_ || failed_) return status;  // the constructor failed: error() says how
  const int n = streams();
  error_.clear(), disagreed = false;
  // every entry's arguments first: a round is refused as a whole
  for (int i = 0; i < n; i++) {
    const BatchEntry &e = entries[i];
    if (e.present && imageArgsBad(e.width, e.height, e.step, e.encoding, e.pixels)) {
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
  BatchRoute route(ctx_);
  if (int rc = settings_.apply(cfg_, f.width, f.height, {f.encoding, f.step}, route)) return status = rc;
  const int tw = trackedWidth(cfg_, f.width), th = trackedHeight(cfg_, f.height);
  for (int i = 0; i < n; i++) {
    const BatchEntry &e = entries[i];
    if (active[i]) buffers_[i].fill(cfg_, tw, th, e.pixels, e.stamp, gate[i].publish, rng_[i], &in_[i], &out_[i], &msg_[i]);
    else in_[i] = LfvioTrackFrameIn();  // image null: the slot is idle in this call
  }
  if (int rc = lfvio_track_batch_frame(ctx_, n, in_.data(), out_.data(), msg_.data())) return status = rc;
  for (int i = 0; i < n; i++) {
    if (!active[i]) continue;
    BatchEntry &e = entries[i];
    e.result = frameResult(gate[i].afterFrame());  // :113-178
    if (e.result == FeatureTracker::PUBLISHED) buffers_[i].message(e.stamp, msg_[i].num_rows, &e.msg);
  }
  return LFVIO_OK;
}

int trackRecordings(BatchFeatureTracker &tracker, int n, const char *const *in_paths, std::vector<std::vector<char>> *outs, TrackStats *stats) {
  if (stats && n > 0) std::memset(stats, 0, (size_t)n * sizeof(TrackStats));
  if (tracker.status != LFVIO_OK) return -2;  // the tracker's constructor failed
  if (n != tracker.streams()) return -3;
  const int rc = rewriteRecordings(n, in_paths, outs, stats, [&](BatchEntry *entries) { return tracker.onRound(entries); });
  return rc == -2 && tracker.disagreed ? -4 : rc;
}

}  // namespace lfvio
