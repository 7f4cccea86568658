// tracker_capi.cpp — extern "C" driver of the image route (feature_tracker.h, batch_tracker.h and image_replay.h, over the recipe of
// track_node.h and the walk of trace_rewrite.h), beside host_capi.cpp and apart from it:
// the test suite's CPU build of the host sources (oracle/Makefile) links no tracker, so nothing in the three older sources refers to
// anything here.  Only host/Makefile compiles this file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "batch_tracker.h"
#include "feature_tracker.h"
#include "image_replay.h"
#include "window_estimator.h"

using namespace lfvio;

namespace {
TrackerConfig &trackerConfig() {  // process-wide, like Config
  static TrackerConfig c;
  return c;
}
std::string &tracesError() {  // of the last lfvio_host_track_traces
  static std::string s;
  return s;
}
inline WindowEstimator *E(void *h) { return (WindowEstimator *)h; }
void give(double *dst, const TrackStats &st) {
  if (dst) std::memcpy(dst, &st, sizeof st);
}
static_assert(sizeof(TrackStats) == 7 * sizeof(double), "track_stats[7]");
}  // namespace

extern "C" {

// The tracker's YAML values.  iv[6] = {MAX_CNT, MIN_DIST, FREQ, EQUALIZE, sample sets of rejectWithF, seed of their generator (0:
// std::random_device)}; the base mask: mask (mask_width x mask_height pixels), else annulus[4] = {center_x, center_y, max_r, min_r},
// else (both null) none.  Used by the next lfvio_host_track_trace / lfvio_host_replay_images.
void lfvio_host_track_config(const LfvioCamera *camera, const int *iv, const double *annulus, int mask_width, int mask_height, const unsigned char *mask) {
  TrackerConfig &c = trackerConfig();
  c = TrackerConfig();
  if (camera) c.camera = *camera;
  c.max_cnt = iv[0], c.min_dist = iv[1], c.freq = iv[2], c.equalize = iv[3] != 0, c.num_samples = iv[4], c.ransac_seed = (unsigned)iv[5];
  if (mask && mask_width > 0 && mask_height > 0) {
    c.mask.assign(mask, mask + (size_t)mask_width * mask_height);
    c.mask_width = mask_width, c.mask_height = mask_height;
  } else if (annulus) {
    c.annulus = true;
    c.center_x = annulus[0], c.center_y = annulus[1], c.max_r = annulus[2], c.min_r = annulus[3];
  }
}

// Track on the expanded image (TrackerConfig::expand, feature_tracker.h): src: the SOURCE camera's projector, or null: off; kind
// LFVIO_MAP_EQUIRECT or LFVIO_MAP_PERSPECTIVE with M[9] (null: zeros); width x height: the image that is tracked, whose camera and
// base mask lfvio_host_track_config then names.  Call it BEHIND lfvio_host_track_config, which starts from a fresh TrackerConfig.
void lfvio_host_track_expand(const LfvioProjector *src, int kind, int width, int height, const double *M) {
  TrackerConfig::Expand &x = trackerConfig().expand;
  x = TrackerConfig::Expand();
  if (!src || !src->camera) return;
  x.on = true, x.kind = kind, x.width = width, x.height = height;
  if (M) std::memcpy(x.M, M, sizeof x.M);
  x.src_camera = *src->camera;
  std::memcpy(x.inv_poly, src->inv_poly, sizeof x.inv_poly);
}

// "Pre-track a bag": the recording in_path with every raw image (record type 10) replaced by what a fresh FeatureTracker on the
// estimator's context emitted for it, every other record copied.  track_stats[7] (or null) = {raw images, dropped, restarts, tracked
// only, published, rows in total, milliseconds in the tracker}.  0; -1 cannot write; -2 a device call failed; -3 unreadable or refused.
int lfvio_host_track_trace(void *h, const char *in_path, const char *out_path, double *track_stats) {
  WindowEstimator *e = E(h);
  if (!e->device()) return -2;
  FeatureTracker tracker(trackerConfig(), e->gpu);
  TrackStats st;
  const int rc = trackTrace(tracker, in_path, out_path, &st);
  give(track_stats, st);
  return rc;
}

// Several recordings through ONE batched tracker call per round (batch_tracker.h): round r takes the r-th raw image of every
// recording that still has one, recording i is slot i of the estimator's context.  Every out_paths[i] is, byte for byte, what
// lfvio_host_track_trace writes for in_paths[i] alone under the same lfvio_host_track_config / lfvio_host_track_expand.
// track_stats[n][7] (or null) as above, per recording (milliseconds: of the rounds the recording took part in).  n in [1, 64].
// 0; -1 cannot write; -2 a device call failed; -3 unreadable, refused, or n outside [1, 64]; -4 the images of a round that reach the
// tracker disagree in width, height, step or encoding.  On anything but 0 NO file is written, and lfvio_host_track_traces_error()
// says why.  Afterwards the estimator's context has no batch reserved and the batch's source, format and CLAHE settings are off.
int lfvio_host_track_traces(void *h, int n, const char *const *in_paths, const char *const *out_paths, double *track_stats) {
  std::string &why = tracesError();
  why.clear();
  WindowEstimator *e = E(h);
  if (!e->device()) {
    why = "no device";
    return -2;
  }
  if (n < 1 || n > LFVIO_TRACK_BATCH_MAX_SLOTS || !in_paths || !out_paths) {
    why = "lfvio_host_track_traces: n outside [1, 64], or null paths";
    return -3;
  }
  BatchFeatureTracker tracker(trackerConfig(), n, e->gpu);
  std::vector<TrackStats> st((size_t)n);
  std::vector<std::vector<char>> bytes;
  const int rc = trackRecordings(tracker, n, in_paths, &bytes, st.data());
  if (track_stats) std::memcpy(track_stats, st.data(), (size_t)n * sizeof(TrackStats));
  if (rc) {
    why = rc == -3 ? "lfvio_host_track_traces: a recording is unreadable or refused" : tracker.error();
    return rc;
  }
  for (int i = 0; i < n; i++) {
    if (writeBytes(out_paths[i], bytes[i])) {
      for (int k = 0; k <= i; k++) std::remove(out_paths[k]);
      why = "lfvio_host_track_traces: cannot write";
      return -1;
    }
  }
  return 0;
}
const char *lfvio_host_track_traces_error(void) { return tracesError().c_str(); }

// Pixels to poses: the same tracking, then replay() on the result in memory.  stats as lfvio_host_replay, track_stats as above.
int lfvio_host_replay_images(void *h, const char *path, const char *traj_path, int max_images, int *stats, double *track_stats) {
  WindowEstimator *e = E(h);
  if (!e->device()) return -2;
  FeatureTracker tracker(trackerConfig(), e->gpu);
  ReplayStats rs;
  TrackStats st;
  const int rc = replayImages(*e, tracker, path, traj_path, max_images, &rs, &st);
  if (stats) std::memcpy(stats, &rs, sizeof rs);
  give(track_stats, st);
  return rc;
}

// the raw images of a trace file as the loader sees them: out[cap][5] = {stamp, width, height, step, offset of the pixels}; returns
// their number, -3: unreadable or refused (the loader's message in err[err_cap], if given).  lfvio_host_trace_raw_encoding: the
// code they share (a file of differing codes is refused), -1 without raw images, -3 as above.
int lfvio_host_trace_raw_images(const char *path, int cap, double *out, char *err, int err_cap) {
  Trace trace;
  if (!trace.load(path)) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", trace.error.c_str());
    return -3;
  }
  for (int k = 0; k < (int)trace.raw_images.size() && k < cap; k++) {
    const TraceRawImage &r = trace.raw_images[k];
    out[5 * k] = r.t, out[5 * k + 1] = r.width, out[5 * k + 2] = r.height, out[5 * k + 3] = r.step, out[5 * k + 4] = (double)r.offset;
  }
  return (int)trace.raw_images.size();
}
int lfvio_host_trace_raw_encoding(const char *path) {
  Trace trace;
  if (!trace.load(path)) return -3;
  return trace.raw_images.empty() ? -1 : (int)trace.raw_images[0].encoding;
}

}  // extern "C"
