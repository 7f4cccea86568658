// track_plan.h — the host side of lfvio_track_reject / lfvio_track_undistort (include/lfvio.h) that needs no device and is not about
// a camera model: the argument checks of both calls (the camera's own check, TrackCam and track_cam are camera_models.h's, included
// here), the sizes of a stream's buffers and the copy of rejectWithF's record.  Plain C++ (no HIP): track.inc uses it,
// tests/test_track_ref.py compiles it alone with g++ and holds it to the checks of tests/track_ref.py.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/lfvio.h"
#include "camera_models.h"

constexpr int TRACK_MAX_SAMPLES = 1024, TRACK_MIN_MATCHES = 8;  // forw_pts.size() >= 8 (feature_tracker.cpp:331)

// A stream's buffers, of either route.  The (id, un_pts_3d) map: [4096 ids | 4096 x 3 floats], the un_pts_3d at TRACK_MAP_IDS.  The
// track table: [4096 x 2 floats | 4096 ids | 4096 counts].
constexpr size_t TRACK_MAP_IDS = (size_t)LFVIO_TRACK_MAX_POINTS * 4, TRACK_MAP_BYTES = TRACK_MAP_IDS + (size_t)LFVIO_TRACK_MAX_POINTS * 12;
constexpr size_t TRACK_TABLE_BYTES = (size_t)LFVIO_TRACK_MAX_POINTS * 16;

// rejectWithF's record from the device's copy.  status != 0 is "no model": E is left as dst had it (the caller's own in
// lfvio_track_reject, zeros in the frame routes, which clear dst first).
inline void track_reject_copy(LfvioTrackRejectOut *dst, const LfvioTrackRejectOut &src) {
  if (src.status == 0)
    *dst = src;
  else
    dst->status = src.status, dst->best_sample = src.best_sample, dst->num_inliers = src.num_inliers, dst->best_score = src.best_score;
}

// nullptr, or what is wrong with the camera (camera_models.h) or the point count
inline const char *track_common_check(const LfvioCamera *cam, int N) {
  if (const char *why = track_camera_check(cam)) return why;
  if (N < 0 || N > LFVIO_TRACK_MAX_POINTS) return "lfvio_track: num_points outside [0, 4096]";
  return nullptr;
}

// nullptr, or what is wrong with *in (the sample sets count only where the device runs: N >= 8)
inline const char *track_reject_check(const LfvioTrackRejectIn *in) {
  if (const char *why = track_common_check(in->camera, in->num_points)) return why;
  const int N = in->num_points, S = in->num_samples;
  if (N > 0 && (!in->cur_pts || !in->forw_pts)) return "lfvio_track_reject: null cur_pts or forw_pts";
  if (N < TRACK_MIN_MATCHES) return nullptr;
  if (S < 1 || S > TRACK_MAX_SAMPLES) return "lfvio_track_reject: num_samples outside [1, 1024]";
  if (!in->samples) return "lfvio_track_reject: null samples";
  for (int k = 0; k < 8 * S; k++)
    if (in->samples[k] < 0 || in->samples[k] >= N) return "lfvio_track_reject: sample index outside [0, num_points)";
  return nullptr;
}

inline const char *track_undistort_check(const LfvioTrackUndistortIn *in) {
  if (const char *why = track_common_check(in->camera, in->num_points)) return why;
  if (in->num_points > 0 && (!in->pts || !in->ids)) return "lfvio_track_undistort: null pts or ids";
  if (std::isnan(in->time)) return "lfvio_track_undistort: time is NaN";
  return nullptr;
}
