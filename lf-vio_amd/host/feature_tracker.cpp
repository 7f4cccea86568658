// feature_tracker.cpp — see feature_tracker.h.  Reference lines are relative to the reference's feature_tracker/src.
#include "feature_tracker.h"

#include "../csrc/image_format.h"

#include <algorithm>
#include <cstring>
#include <functional>

namespace lfvio {

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
  if (cfg_.ransac_seed != 0) {
    rng_.seed(cfg_.ransac_seed);
  } else {  // as WindowEstimator::seedRansac (random_array.cc:12-19)
    std::random_device rd;
    std::vector<std::uint_least32_t> v(10);
    std::generate(v.begin(), v.end(), std::ref(rd));
    std::seed_seq seq(v.begin(), v.end());
    rng_.seed(seq);
  }
  const size_t cap = LFVIO_TRACK_MAX_POINTS;
  pts_.resize(cap * 2), un_pts_.resize(cap * 2), un_pts_3d_.resize(cap * 3), velocity_3d_.resize(cap * 3), rows_.resize(cap * 9);
  ids_.resize(cap), track_cnt_.resize(cap);
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
  const LfvioImageFormat format = {encoding, step};
  if (!pixels || !msg || width < 1 || height < 1 || step < 1 || imgfmt_check(format, width, height)) {
    error_ = "FeatureTracker::onImage: null pixels or msg, an unknown encoding, or step < width * bytes per pixel";
    return status = LFVIO_ERR_ARG;
  }
  const ImageGate::Stamp what = gate.onStamp(stamp);  // feature_tracker_node.cpp:30-62
  if (what == ImageGate::DROP) return DROPPED;
  if (what == ImageGate::RESTART) return RESTART;
  // the image that is tracked: the record's, or the expanded one that the device gathers from it
  const TrackerConfig::Expand &ex = cfg_.expand;
  const int tw = ex.on ? ex.width : width, th = ex.on ? ex.height : height;
  const LfvioTrackSource source = {width, height};
  if (!ready_) {  // the base mask (feature_tracker.cpp:53-56) and EQUALIZE (:101-107), once
    int rc = LFVIO_OK;
    if (!cfg_.mask.empty()) {
      rc = lfvio_gft_set_mask(ctx_, cfg_.mask_width, cfg_.mask_height, cfg_.mask.data());
    } else if (cfg_.annulus) {
      std::vector<unsigned char> m((size_t)tw * th);
      const double hi = cfg_.max_r * cfg_.max_r, lo = cfg_.min_r * cfg_.min_r;
      for (int y = 0; y < th; y++)
        for (int x = 0; x < tw; x++) {
          const double dx = x - cfg_.center_x, dy = y - cfg_.center_y, d2 = dx * dx + dy * dy;
          m[(size_t)y * tw + x] = d2 <= hi && d2 > lo ? 255 : 0;
        }
      rc = lfvio_gft_set_mask(ctx_, tw, th, m.data());
    } else {
      rc = lfvio_gft_set_mask(ctx_, 0, 0, nullptr);
    }
    if (rc == LFVIO_OK) {
      const LfvioClaheIn clahe = {3.0, 8, 8};
      rc = lfvio_clahe_set(ctx_, cfg_.equalize ? &clahe : nullptr);
    }
    if (rc == LFVIO_OK) rc = lfvio_image_format_set(ctx_, &format);  // (mono8 with step == width: the same as none)
    if (rc == LFVIO_OK && ex.on) {  // the map of the expanded image through the source camera, resident from here on
      LfvioProjector proj = {};
      proj.camera = &ex.src_camera;
      std::memcpy(proj.inv_poly, ex.inv_poly, sizeof proj.inv_poly);
      LfvioRemapIn rin = {};
      rin.proj = &proj, rin.kind = ex.kind, rin.width = ex.width, rin.height = ex.height;
      std::memcpy(rin.M, ex.M, sizeof rin.M);
      rc = lfvio_remap_build(ctx_, &rin, nullptr, nullptr);
    }
    if (rc == LFVIO_OK) rc = lfvio_track_source_set(ctx_, ex.on ? &source : nullptr);  // (off: whatever an earlier tracker left on the context)
    if (rc != LFVIO_OK) return status = rc;
    format_ = format, source_ = source, ready_ = true;
  }
  if (ex.on && (source.src_width != source_.src_width || source.src_height != source_.src_height)) {  // a driver that changes its size
    if (int rc = lfvio_track_source_set(ctx_, &source)) return status = rc;
    source_ = source;
  }
  if (format.encoding != format_.encoding || format.step != format_.step) {  // a driver that changes its rows
    if (int rc = lfvio_image_format_set(ctx_, &format)) return status = rc;
    format_ = format;
  }
  const unsigned char *image = pixels;  // height rows of step bytes: no repacking on the host (with expand: the SOURCE image)
  const bool pub = gate.publish;
  const int S = cfg_.num_samples;
  if (pub) {  // num_samples x 8 raw outputs of the generator, row-major; nothing is drawn for a frame that is only tracked
    words_.resize((size_t)std::max(S, 0) * 8);
    for (unsigned &w : words_) w = (unsigned)rng_();
  }
  LfvioTrackFrameIn in = {};
  in.width = tw, in.height = th, in.image = image, in.time = stamp, in.publish = pub ? 1 : 0, in.camera = &cfg_.camera;
  in.win_size = 41, in.max_level = 3, in.max_iterations = 30, in.epsilon = 0.01, in.min_eig_threshold = 1e-4, in.border = 1;  // feature_tracker.cpp:127
  in.max_count = cfg_.max_cnt, in.quality_level = 0.01, in.min_distance = cfg_.min_dist, in.mask_radius = cfg_.min_dist;  // :60-75, :157
  in.num_samples = S, in.sample_words = pub ? words_.data() : nullptr, in.capacity = LFVIO_TRACK_MAX_POINTS;
  LfvioTrackFrameOut out = {};
  out.pts = pts_.data(), out.ids = ids_.data(), out.track_cnt = track_cnt_.data();
  out.un_pts = un_pts_.data(), out.un_pts_3d = un_pts_3d_.data(), out.velocity_3d = velocity_3d_.data();
  LfvioTrackMessage m = {0, rows_.data()};
  const int rc = lfvio_track_frame_message(ctx_, &in, &out, nullptr, &m);
  if (rc != LFVIO_OK) return status = rc;
  last_points = out.num_points;
  const ImageGate::Frame after = gate.afterFrame();  // :113-178
  if (after == ImageGate::TRACKED_ONLY) return TRACKED_ONLY;
  if (after == ImageGate::FIRST_PUBLICATION) return FIRST_PUBLICATION_SKIPPED;
  msg->t = stamp;
  msg->v.assign(rows_.begin(), rows_.begin() + (size_t)m.num_rows * 9);
  return PUBLISHED;
}

}  // namespace lfvio
