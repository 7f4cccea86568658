// feature_tracker.cpp — see feature_tracker.h.  The node's recipe is track_node.h's; this file holds the single tracker's device calls.
// Reference lines are relative to the reference's feature_tracker/src.
#include "feature_tracker.h"

namespace lfvio {

namespace {
struct ContextRoute final : SettingsRoute {  // the settings of the context itself
  lfvio_ctx *ctx;
  explicit ContextRoute(lfvio_ctx *c) : ctx(c) {}
  int mask(int width, int height, const unsigned char *pixels) override { return lfvio_gft_set_mask(ctx, width, height, pixels); }
  int clahe(const LfvioClaheIn *clahe) override { return lfvio_clahe_set(ctx, clahe); }
  int format(const LfvioImageFormat *format) override { return lfvio_image_format_set(ctx, format); }
  int map(const LfvioRemapIn *in) override { return lfvio_remap_build(ctx, in, nullptr, nullptr); }
  int source(const LfvioTrackSource *source) override { return lfvio_track_source_set(ctx, source); }
};
}  // namespace

FeatureTracker::FeatureTracker(const TrackerConfig &config, lfvio_ctx *ctx, int device) : cfg_(config), ctx_(ctx) {
  gate.freq = cfg_.freq;
  if (!ctx_) {
    ctx_ = lfvio_create(device);
    own_ = ctx_ != nullptr;
  }
  if (!ctx_) {
    status = LFVIO_ERR_DEVICE;  // there is no host fallback: every onImage returns it
    error_ = "lfvio_create failed";
    return;
  }
  status = lfvio_track_frame_reset(ctx_);
  seedSamples(rng_, cfg_.ransac_seed);
}

FeatureTracker::~FeatureTracker() {
  if (own_) lfvio_destroy(ctx_);
}

const char *FeatureTracker::error() const { return ctx_ && error_.empty() ? lfvio_last_error(ctx_) : error_.c_str(); }

int FeatureTracker::onImage(double stamp, int width, int height, int step, const unsigned char *pixels, TraceImage *msg) {
  return onImage(stamp, width, height, step, LFVIO_IMG_MONO8, pixels, msg);
}

int FeatureTracker::onImage(double stamp, int width, int height, int step, int encoding, const unsigned char *pixels, TraceImage *msg) {
  if (!ctx_) return status;
  if (!msg || imageArgsBad(width, height, step, encoding, pixels)) {
    error_ = "FeatureTracker::onImage: null pixels or msg, an unknown encoding, or step < width * bytes per pixel";
    return status = LFVIO_ERR_ARG;
  }
  const ImageGate::Stamp what = gate.onStamp(stamp);  // feature_tracker_node.cpp:30-62
  if (what == ImageGate::DROP) return DROPPED;
  if (what == ImageGate::RESTART) return RESTART;
  ContextRoute route(ctx_);
  if (int rc = settings_.apply(cfg_, width, height, {encoding, step}, route)) return status = rc;
  LfvioTrackFrameIn in;
  LfvioTrackFrameOut out;
  LfvioTrackMessage m;
  buffers_.fill(cfg_, trackedWidth(cfg_, width), trackedHeight(cfg_, height), pixels, stamp, gate.publish, rng_, &in, &out, &m);
  if (int rc = lfvio_track_frame_message(ctx_, &in, &out, nullptr, &m)) return status = rc;
  last_points = out.num_points;
  const int result = frameResult(gate.afterFrame());  // :113-178
  if (result == PUBLISHED) buffers_.message(stamp, m.num_rows, msg);
  return result;
}

}  // namespace lfvio
