// batch_tracker.h — N feature tracker nodes on the host around ONE device call per round of images, lfvio_track_batch_frame
// (include/lfvio.h): stream i is slot i of the context's batch, with an ImageGate (image_gate.h) and a generator of rejectWithF's
// sample sets of its own, seeded as FeatureTracker's (feature_tracker.h) is — so stream i publishes what a FeatureTracker alone would
// have published for its images, bit for bit (the batch's contract).  The base mask, the CLAHE setting, the image format and, where
// asked for, the map of the expanded image in every slot (lfvio_track_batch_map) with lfvio_track_batch_source are set at the first
// round that reaches the device.  As in FeatureTracker, a restart resets nothing of the slot: the reference's node does not either.
// The contract holds by construction: the seeding, the mask, the order of the settings, the arguments of every slot with the
// reference's constants and the results are track_node.h's, for both trackers; the batch's own are the round refused as a whole, the
// agreement of a round's images, the idle slots and a destructor that turns the batch's settings off.
// Only host/Makefile builds it.
#pragma once
#include <random>
#include <string>
#include <vector>

#include "../../include/lfvio.h"
#include "feature_tracker.h"
#include "image_gate.h"
#include "trace_rewrite.h"
#include "track_node.h"

namespace lfvio {

class BatchFeatureTracker {
 public:
  // ctx: the context to run on, or null for one of its own on `device`.  The context's batch is reserved anew: every stream starts
  // empty.  streams in [1, LFVIO_TRACK_BATCH_MAX_SLOTS].  A constructor that fails (streams, lfvio_create, the reservation) leaves
  // `status` and error(), and every onRound returns that status.  The destructor frees the batch and turns the batch's source, format
  // and CLAHE settings off again, so a caller's context is left as a fresh one's as far as the batch goes.
  BatchFeatureTracker(const TrackerConfig &config, int streams, lfvio_ctx *ctx = nullptr, int device = 0);
  ~BatchFeatureTracker();
  BatchFeatureTracker(const BatchFeatureTracker &) = delete;
  BatchFeatureTracker &operator=(const BatchFeatureTracker &) = delete;

  // One round: entries[streams].  The streams whose gate lets their image through make ONE lfvio_track_batch_frame; the others are
  // idle in it.  Returns LFVIO_OK with every present entry's result set, or a negative status (`status`, error()): LFVIO_ERR_ARG
  // where an entry is malformed or the images that reach the tracker disagree in width, height, step or encoding (nothing has
  // reached the device then), otherwise the status of the device call that failed.  No silent continuation.
  int onRound(BatchEntry *entries);

  const char *error() const;
  int status = LFVIO_OK;
  bool disagreed = false;  // the last onRound was refused because its images disagree
  int streams() const { return (int)gate.size(); }
  std::vector<ImageGate> gate;

 private:
  TrackerConfig cfg_;
  lfvio_ctx *ctx_ = nullptr;
  bool own_ = false, failed_ = false;
  std::vector<std::mt19937> rng_;
  NodeSettings settings_;  // of every slot
  std::vector<FrameBuffers> buffers_;
  std::vector<LfvioTrackFrameIn> in_;
  std::vector<LfvioTrackFrameOut> out_;
  std::vector<LfvioTrackMessage> msg_;
  std::string error_;
};

// n recordings walked in lockstep — round r takes the r-th raw image (record type 10) of every recording that still has one — through
// `tracker` (n streams): outs[i] is recording i as image_replay.h's trackRecording makes it alone, the bytes of an LFVT file; stats[n].
// 0; -3: a recording is unreadable or refused by Trace::load; -2: a device call failed; -4: the images of a round that reach the
// tracker disagree in width, height, step or encoding (tracker.error() either way).  On anything but 0 the outs are not to be used.
int trackRecordings(BatchFeatureTracker &tracker, int n, const char *const *in_paths, std::vector<std::vector<char>> *outs, TrackStats *stats);

}  // namespace lfvio
