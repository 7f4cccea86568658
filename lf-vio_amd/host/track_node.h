// track_node.h — the feature tracker node's recipe, stated once for FeatureTracker (feature_tracker.h) and BatchFeatureTracker
// (batch_tracker.h): the YAML values, the generator's seeding, the base mask, the map of the expanded image, the check of one image's
// arguments, the arguments of one readImage with the reference's constants, the results, and the order of the context's settings at
// the first image and behind a driver that changes its rows or its size.  Header-only and without a device symbol: the five device
// calls of the settings go through a SettingsRoute that each tracker implements in its own source, so that stream i of the batch
// publishes what a FeatureTracker alone would by construction.  tests/test_track_node.py compiles it alone with g++.
// Reference lines are relative to the reference's feature_tracker/src.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/lfvio.h"
#include "../csrc/image_format.h"
#include "image_gate.h"
#include "replay.h"

namespace lfvio {

struct TrackerConfig {
  LfvioCamera camera = {};
  int max_cnt = 150;   // MAX_CNT
  int min_dist = 30;   // MIN_DIST: goodFeaturesToTrack's distance and the radius of setMask's discs
  int freq = 10;       // FREQ
  bool equalize = false;  // EQUALIZE: CLAHE (3.0, 8 x 8) before the pyramid
  // the base mask (fisheye_mask): pixels of the image's size, or the annulus min_r^2 < (x - center_x)^2 + (y - center_y)^2 <= max_r^2
  // rasterised at the first image (Euclidean discs, as lfvio.engine.annulus_mask), or neither: every pixel allowed
  std::vector<unsigned char> mask;
  int mask_width = 0, mask_height = 0;
  bool annulus = false;
  double center_x = 0, center_y = 0, max_r = 0, min_r = 0;
  int num_samples = 100;     // rejectWithF's sample sets
  unsigned ransac_seed = 0;  // 0: seeded from std::random_device, as Config::ransac_seed
  // Track on the EXPANDED image (the launch files' remap of pointcloud_image_fusion's equal_rectangle_img onto /camera/image_raw;
  // lfvio_track_source_set): the records stay the raw source images, the map through the SOURCE camera is built at the first image,
  // and `camera` above is then the camera of the width x height image that is tracked — LFVIO_CAM_EQUIRECT for kind
  // LFVIO_MAP_EQUIRECT, a distortion-free LFVIO_CAM_PINHOLE for LFVIO_MAP_PERSPECTIVE — whose size the base mask has too
  struct Expand {
    bool on = false;
    int kind = LFVIO_MAP_EQUIRECT, width = 0, height = 0;
    double M[9] = {};                                  // PERSPECTIVE only
    LfvioCamera src_camera = {};                       // the source camera's LfvioProjector values
    double inv_poly[LFVIO_OCAM_INV_POLY_SIZE] = {};
  } expand;
};

// What became of one image.  FeatureTracker derives from it: FeatureTracker::DROPPED and the others are these.
struct TrackResults {
  enum Result { DROPPED = 0, RESTART = 1, TRACKED_ONLY = 2, FIRST_PUBLICATION_SKIPPED = 3, PUBLISHED = 4 };
};

// the generator of rejectWithF's sample sets: `seed`, or (0) ten words of std::random_device, as WindowEstimator::seedRansac
// (random_array.cc:12-19)
inline void seedSamples(std::mt19937 &rng, unsigned seed) {
  if (seed != 0) {
    rng.seed(seed);
    return;
  }
  std::random_device rd;
  std::vector<std::uint_least32_t> v(10);
  std::generate(v.begin(), v.end(), std::ref(rd));
  std::seed_seq seq(v.begin(), v.end());
  rng.seed(seq);
}

// the image that is tracked: the record's, or the expanded one that the device gathers from it
inline int trackedWidth(const TrackerConfig &cfg, int width) { return cfg.expand.on ? cfg.expand.width : width; }
inline int trackedHeight(const TrackerConfig &cfg, int height) { return cfg.expand.on ? cfg.expand.height : height; }

// The base mask of a tw x th tracked image (feature_tracker.cpp:53-56): the given one, the annulus rasterised into *storage, or
// {0, 0, null}: none
struct BaseMask {
  int width, height;
  const unsigned char *pixels;
};
inline BaseMask baseMask(const TrackerConfig &cfg, int tw, int th, std::vector<unsigned char> *storage) {
  if (!cfg.mask.empty()) return {cfg.mask_width, cfg.mask_height, cfg.mask.data()};
  if (!cfg.annulus) return {0, 0, nullptr};
  storage->resize((size_t)tw * th);
  const double hi = cfg.max_r * cfg.max_r, lo = cfg.min_r * cfg.min_r;
  for (int y = 0; y < th; y++)
    for (int x = 0; x < tw; x++) {
      const double dx = x - cfg.center_x, dy = y - cfg.center_y, d2 = dx * dx + dy * dy;
      (*storage)[(size_t)y * tw + x] = d2 <= hi && d2 > lo ? 255 : 0;
    }
  return {tw, th, storage->data()};
}

// the map of the expanded image through the source camera: `in` points into this object and into `ex`
struct ExpandMap {
  LfvioProjector proj = {};
  LfvioRemapIn in = {};
  explicit ExpandMap(const TrackerConfig::Expand &ex) {
    proj.camera = &ex.src_camera;
    std::memcpy(proj.inv_poly, ex.inv_poly, sizeof proj.inv_poly);
    in.proj = &proj, in.kind = ex.kind, in.width = ex.width, in.height = ex.height;
    std::memcpy(in.M, ex.M, sizeof in.M);
  }
  ExpandMap(const ExpandMap &) = delete;
  ExpandMap &operator=(const ExpandMap &) = delete;
};

// one image's arguments: null pixels, an unknown encoding, or step < width * bytes per pixel
inline bool imageArgsBad(int width, int height, int step, int encoding, const unsigned char *pixels) {
  const LfvioImageFormat format = {encoding, step};
  return !pixels || width < 1 || height < 1 || step < 1 || imgfmt_check(format, width, height);
}

// img_callback behind readImage (feature_tracker_node.cpp:113-178)
inline int frameResult(ImageGate::Frame after) {
  if (after == ImageGate::TRACKED_ONLY) return TrackResults::TRACKED_ONLY;
  if (after == ImageGate::FIRST_PUBLICATION) return TrackResults::FIRST_PUBLICATION_SKIPPED;
  return TrackResults::PUBLISHED;
}

// One stream's host memory around readImage: the seven arrays a call writes and the sample words it reads
struct FrameBuffers {
  std::vector<float> pts, un_pts, un_pts_3d, velocity_3d, rows;
  std::vector<int> ids, track_cnt;
  std::vector<unsigned> words;
  FrameBuffers() {
    const size_t cap = LFVIO_TRACK_MAX_POINTS;
    pts.resize(cap * 2), un_pts.resize(cap * 2), un_pts_3d.resize(cap * 3), velocity_3d.resize(cap * 3), rows.resize(cap * 9);
    ids.resize(cap), track_cnt.resize(cap);
  }
  // The arguments of one readImage of the tw x th image behind `pixels` (height rows of step bytes: no repacking on the host; with
  // expand the SOURCE image).  publish: num_samples x 8 raw outputs of the stream's generator, row-major; nothing is drawn for a frame
  // that is only tracked.  *in points into cfg and into this object.
  void fill(const TrackerConfig &cfg, int tw, int th, const unsigned char *pixels, double stamp, bool publish, std::mt19937 &rng, LfvioTrackFrameIn *in,
            LfvioTrackFrameOut *out, LfvioTrackMessage *msg) {
    const int S = cfg.num_samples;
    if (publish) {
      words.resize((size_t)std::max(S, 0) * 8);
      for (unsigned &w : words) w = (unsigned)rng();
    }
    *in = LfvioTrackFrameIn();
    in->width = tw, in->height = th, in->image = pixels, in->time = stamp, in->publish = publish ? 1 : 0, in->camera = &cfg.camera;
    in->win_size = 41, in->max_level = 3, in->max_iterations = 30, in->epsilon = 0.01, in->min_eig_threshold = 1e-4, in->border = 1;  // feature_tracker.cpp:127
    in->max_count = cfg.max_cnt, in->quality_level = 0.01, in->min_distance = cfg.min_dist, in->mask_radius = cfg.min_dist;  // :60-75, :157
    in->num_samples = S, in->sample_words = publish ? words.data() : nullptr, in->capacity = LFVIO_TRACK_MAX_POINTS;
    *out = LfvioTrackFrameOut();
    out->pts = pts.data(), out->ids = ids.data(), out->track_cnt = track_cnt.data();
    out->un_pts = un_pts.data(), out->un_pts_3d = un_pts_3d.data(), out->velocity_3d = velocity_3d.data();
    msg->num_rows = 0, msg->rows = rows.data();
  }
  // the feature message of a PUBLISHED frame
  void message(double stamp, int num_rows, TraceImage *msg) const {
    msg->t = stamp;
    msg->v.assign(rows.begin(), rows.begin() + (size_t)num_rows * 9);
  }
};

// The five settings of a context (or of every slot of its batch) that the node makes; each returns the device call's status
struct SettingsRoute {
  virtual int mask(int width, int height, const unsigned char *pixels) = 0;
  virtual int clahe(const LfvioClaheIn *clahe) = 0;
  virtual int format(const LfvioImageFormat *format) = 0;
  virtual int map(const LfvioRemapIn *in) = 0;
  virtual int source(const LfvioTrackSource *source) = 0;

 protected:
  ~SettingsRoute() = default;
};

struct NodeSettings {
  bool ready_ = false;
  LfvioImageFormat format_ = {LFVIO_IMG_MONO8, 0};  // what the context's format was last set to (ready_)
  LfvioTrackSource source_ = {0, 0};                // ... and, with cfg.expand.on, its source

  // Before readImage of a width x height image in `format`.  At the first use the base mask (feature_tracker.cpp:53-56), EQUALIZE
  // (:101-107), the format (mono8 with step == width: the same as none), with expand the map of the expanded image, resident from
  // here on, and the source (off: null, which turns off whatever an earlier tracker left on the context); later a source or a format
  // that changed.  Stops at the first status that is not LFVIO_OK and returns it; a first use that failed is repeated as a whole.
  int apply(const TrackerConfig &cfg, int width, int height, const LfvioImageFormat &format, SettingsRoute &route) {
    const TrackerConfig::Expand &ex = cfg.expand;
    const LfvioTrackSource source = {width, height};
    if (!ready_) {
      std::vector<unsigned char> storage;
      const BaseMask m = baseMask(cfg, trackedWidth(cfg, width), trackedHeight(cfg, height), &storage);
      if (int rc = route.mask(m.width, m.height, m.pixels)) return rc;
      const LfvioClaheIn clahe = {3.0, 8, 8};
      if (int rc = route.clahe(cfg.equalize ? &clahe : nullptr)) return rc;
      if (int rc = route.format(&format)) return rc;
      if (ex.on) {
        const ExpandMap map(ex);
        if (int rc = route.map(&map.in)) return rc;
      }
      if (int rc = route.source(ex.on ? &source : nullptr)) return rc;
      format_ = format, source_ = source, ready_ = true;
    }
    if (ex.on && (source.src_width != source_.src_width || source.src_height != source_.src_height)) {  // a driver that changes its size
      if (int rc = route.source(&source)) return rc;
      source_ = source;
    }
    if (format.encoding != format_.encoding || format.step != format_.step) {  // a driver that changes its rows
      if (int rc = route.format(&format)) return rc;
      format_ = format;
    }
    return LFVIO_OK;
  }
};

}  // namespace lfvio
