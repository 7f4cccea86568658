// image_replay.h — recordings with raw images (record type 10 of replay.h): the FeatureTracker of feature_tracker.h over the images in
// file order, every image replaced by what the node would have published at that place — a feature message (type 2), a restart
// (type 5, with the stamp) or nothing — and every other record copied byte for byte.  trackTrace() writes that recording ("pre-track
// a bag"); replayImages() makes it in memory and hands it to the unchanged replay(): pixels and IMU samples in, the trajectory out.
// The walk over the records, TrackStats and the file writing are trace_rewrite.h's, shared with batch_tracker.h's trackRecordings.
#pragma once
#include <vector>

#include "feature_tracker.h"
#include "replay.h"
#include "trace_rewrite.h"

namespace lfvio {

// The recording `in_path` with its raw images tracked, as the bytes of an LFVT file in *out.  0; -3: unreadable or refused by
// Trace::load; -2: a device call of the tracker failed (tracker.status, tracker.error()).
int trackRecording(FeatureTracker &tracker, const char *in_path, std::vector<char> *out, TrackStats *stats);

// ... written to out_path.  -1: cannot write.
int trackTrace(FeatureTracker &tracker, const char *in_path, const char *out_path, TrackStats *stats);

// ... loaded as a Trace and replayed: replay() of replay.h on the result, its return values and `stats`.
int replayImages(WindowEstimator &estimator, FeatureTracker &tracker, const char *path, const char *traj_path, int max_images, ReplayStats *stats,
                 TrackStats *track_stats, std::vector<double> *image_ms = nullptr);

}  // namespace lfvio
