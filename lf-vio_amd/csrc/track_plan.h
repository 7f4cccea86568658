// track_plan.h — the host side of lfvio_track_reject / lfvio_track_undistort (include/lfvio.h) that needs no device: the argument
// checks of both calls, and the camera as the kernels take it (TrackCam: LfvioCamera's numbers with inv_scale = 1.0 / (c - d * e),
// divided once, on the host, in double — ScaramuzzaCamera.cc:197).  Plain C++ (no HIP): track.inc uses it, tests/test_track_ref.py
// compiles it alone with g++ and holds it to the checks of tests/track_ref.py.
#pragma once
#include <cmath>

#include "../../include/lfvio.h"

constexpr int TRACK_MAX_SAMPLES = 1024, TRACK_MIN_MATCHES = 8;  // forw_pts.size() >= 8 (feature_tracker.cpp:331)

struct TrackCam {  // a kernel argument, by value
  double cx, cy, c, d, e, inv_scale, poly[5];
};

inline TrackCam track_cam(const LfvioCamera &k) {
  TrackCam t;
  t.cx = k.cx, t.cy = k.cy, t.c = k.c, t.d = k.d, t.e = k.e;
  t.inv_scale = 1.0 / (k.c - k.d * k.e);
  for (int i = 0; i < 5; i++) t.poly[i] = k.poly[i];
  return t;
}

// nullptr, or what is wrong with the camera or the point count
inline const char *track_common_check(const LfvioCamera *cam, int N) {
  if (!cam) return "lfvio_track: null camera";
  if (cam->model != LFVIO_CAM_OCAM) return "lfvio_track: a camera model other than LFVIO_CAM_OCAM";
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
