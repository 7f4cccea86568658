// tracker_capi.cpp — extern "C" driver of the image route (feature_tracker.h, image_replay.h), beside host_capi.cpp and apart from it:
// the test suite's CPU build of the host sources (oracle/Makefile) links no tracker, so nothing in the three older sources refers to
// anything here.  Only host/Makefile compiles this file.
#include <cstring>

#include "feature_tracker.h"
#include "image_replay.h"
#include "window_estimator.h"

using namespace lfvio;

namespace {
TrackerConfig &trackerConfig() {  // process-wide, like Config
  static TrackerConfig c;
  return c;
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
