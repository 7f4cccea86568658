// feature_tracker.h — the feature tracker node on the host: img_callback (feature_tracker/src/feature_tracker_node.cpp:28-178) around ONE
// device call per image, lfvio_track_frame_message (include/lfvio.h), which runs readImage, updateID and the feature message on a
// track table resident in the context.  What is left here is the node's bookkeeping (image_gate.h), the base mask, the CLAHE setting and
// the image format (lfvio_image_format_set: the record's rows go up as they are, padded, colour or 16-bit, and the device makes grey
// of them) at the first use, where asked for the map of the expanded image and lfvio_track_source_set beside them, and the generator
// of rejectWithF's sample sets.  The recipe of all that — the YAML values (TrackerConfig), the seeding, the mask, the settings' order,
// the arguments of the device call with the reference's constants, the results — is track_node.h's, which BatchFeatureTracker
// (batch_tracker.h) follows too; here are the context, the gate, the device calls and the class.
// Not compiled into the test suite's CPU build of the host sources (oracle/Makefile): only host/Makefile builds it.
#pragma once
#include <random>
#include <string>
#include <vector>

#include "../../include/lfvio.h"
#include "image_gate.h"
#include "replay.h"
#include "track_node.h"

namespace lfvio {

class FeatureTracker : public TrackResults {  // Result: DROPPED, RESTART, TRACKED_ONLY, FIRST_PUBLICATION_SKIPPED, PUBLISHED
 public:
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
  bool own_ = false;
  std::mt19937 rng_;
  NodeSettings settings_;
  FrameBuffers buffers_;
  std::string error_;
};

}  // namespace lfvio
