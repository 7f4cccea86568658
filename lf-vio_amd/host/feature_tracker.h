// feature_tracker.h — the feature tracker node on the host: img_callback (feature_tracker/src/feature_tracker_node.cpp:28-178) around ONE
// device call per image, lfvio_track_frame_message (include/lfvio.h), which runs readImage, updateID and the feature message on a
// track table resident in the context.  What is left here is the node's bookkeeping (image_gate.h), the base mask, the CLAHE setting and
// the image format (lfvio_image_format_set: the record's rows go up as they are, padded, colour or 16-bit, and the device makes grey
// of them) at the first use, where asked for the map of the expanded image and lfvio_track_source_set beside them, and the generator
// of rejectWithF's sample sets.
// Not compiled into the test suite's CPU build of the host sources (oracle/Makefile): only host/Makefile builds it.
#pragma once
#include <random>
#include <string>
#include <vector>

#include "../../include/lfvio.h"
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

class FeatureTracker {
 public:
  enum Result { DROPPED = 0, RESTART = 1, TRACKED_ONLY = 2, FIRST_PUBLICATION_SKIPPED = 3, PUBLISHED = 4 };
  // ctx: the context to run on (the estimator's), or null for one of its own on `device`.  The track table, the pyramid and the map of
  // the context are reset: a tracker starts empty.
  explicit FeatureTracker(const TrackerConfig &config, lfvio_ctx *ctx = nullptr, int device = 0);
  ~FeatureTracker();
  FeatureTracker(const FeatureTracker &) = delete;
  FeatureTracker &operator=(const FeatureTracker &) = delete;

  // One sensor_msgs/Image (mono8, `step` bytes per row).  Returns a Result, or the negative status of the device call that failed
  // (`status`, error()): no silent continuation.  PUBLISHED: *msg is the feature message, stamped `stamp`; otherwise msg is untouched.
  int onImage(double stamp, int width, int height, int step, const unsigned char *pixels, TraceImage *msg);
  // ... in the encoding `encoding` (LFVIO_IMG_*, the type-10 record's code): height rows of `step` bytes, handed over as they are
  int onImage(double stamp, int width, int height, int step, int encoding, const unsigned char *pixels, TraceImage *msg);

  const char *error() const;
  int status = LFVIO_OK;
  int last_points = 0;  // the table's count after the last image that reached the tracker
  ImageGate gate;

 private:
  TrackerConfig cfg_;
  lfvio_ctx *ctx_ = nullptr;
  bool own_ = false, ready_ = false;
  std::mt19937 rng_;
  LfvioImageFormat format_ = {LFVIO_IMG_MONO8, 0};  // what the context's format was last set to (ready_)
  LfvioTrackSource source_ = {0, 0};                // ... and, with cfg_.expand.on, its source
  std::vector<unsigned> words_;
  std::vector<float> pts_, un_pts_, un_pts_3d_, velocity_3d_, rows_;
  std::vector<int> ids_, track_cnt_;
  std::string error_;
};

}  // namespace lfvio
