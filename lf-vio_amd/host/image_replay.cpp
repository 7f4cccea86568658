// image_replay.cpp — see image_replay.h.  The walk over the records is trace_rewrite.cpp's, here with one recording.
#include "image_replay.h"

#include <cstdio>
#include <cstring>

namespace lfvio {

int trackRecording(FeatureTracker &tracker, const char *in_path, std::vector<char> *out, TrackStats *stats) {
  std::vector<std::vector<char>> outs;
  const int rc = rewriteRecordings(1, &in_path, &outs, stats, [&](BatchEntry *e) {
    const int what = tracker.onImage(e->stamp, e->width, e->height, e->step, e->encoding, e->pixels, &e->msg);
    if (what >= 0) e->result = what;
    return what;  // negative: a device call failed
  });
  if (!outs.empty()) out->swap(outs[0]);
  return rc;
}

int trackTrace(FeatureTracker &tracker, const char *in_path, const char *out_path, TrackStats *stats) {
  std::vector<char> bytes;
  if (int rc = trackRecording(tracker, in_path, &bytes, stats)) return rc;
  return writeBytes(out_path, bytes);
}

int replayImages(WindowEstimator &estimator, FeatureTracker &tracker, const char *path, const char *traj_path, int max_images, ReplayStats *stats,
                 TrackStats *track_stats, std::vector<double> *image_ms) {
  if (stats) std::memset(stats, 0, sizeof *stats);
  std::vector<char> bytes;
  if (int rc = trackRecording(tracker, path, &bytes, track_stats)) {
    if (stats && rc == -2) stats->last_status = tracker.status;
    return rc;
  }
  std::FILE *f = fmemopen(bytes.data(), bytes.size(), "rb");
  if (!f) return -3;
  Trace trace;
  const bool ok = trace.read(f);
  std::fclose(f);
  if (!ok) return -3;
  return replay(estimator, trace, traj_path, max_images, stats, image_ms);
}

}  // namespace lfvio
