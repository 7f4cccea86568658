// track_plan.h — the host side of lfvio_track_reject / lfvio_track_undistort (include/lfvio.h) that needs no device: the argument
// checks of both calls, and the camera as the kernels take it (TrackCam: LfvioCamera's numbers with inv_scale = 1.0 / (c - d * e),
// divided once, on the host, in double — ScaramuzzaCamera.cc:197; for PINHOLE and MEI the inverse projection matrix's four entries
// and the no-distortion flag, PinholeCamera.cc:281-289; for KANNALA_BRANDT the same four entries and the monotone range of camera_kb.h,
// kept in a KbCache while the camera's numbers stay the same).  Plain C++ (no HIP): track.inc uses it, tests/test_track_ref.py
// compiles it alone with g++ and holds it to the checks of tests/track_ref.py.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/lfvio.h"
#include "camera_kb.h"

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

struct TrackCam {  // a kernel argument, by value; the members a model does not use are zero
  double cx, cy, c, d, e, inv_scale, poly[5];          // OCam
  double inv11, inv13, inv22, inv23, k1, k2, p1, p2, xi;  // PINHOLE and MEI (xi: MEI), PinholeCamera.cc:281-289
  int model, no_distortion;
  double theta_lim, r_lim;  // KANNALA_BRANDT (camera_kb.h), with inv11 .. inv23 and k2 .. k5 in poly[0 .. 3]
};

// LfvioCamera's fx .. xi are read only for PINHOLE and MEI, its c, d, e, poly only for OCam; KANNALA_BRANDT reads cx, cy, fx, fy and
// poly[0 .. 3]: callers may leave the others indeterminate.  kb: where a KANNALA_BRANDT camera's constants are kept from one call to
// the next (nullptr: formed anew); no other model looks at it.
inline TrackCam track_cam(const LfvioCamera &k, KbCache *kb = nullptr) {
  TrackCam t = {};
  t.model = k.model, t.cx = k.cx, t.cy = k.cy;
  if (k.model == LFVIO_CAM_KANNALA_BRANDT) {
    const double key[8] = {k.cx, k.cy, k.fx, k.fy, k.poly[0], k.poly[1], k.poly[2], k.poly[3]};
    KbCache once;
    const KbConstants &c = (kb ? *kb : once).get(key);
    t.inv11 = 1.0 / k.fx, t.inv13 = -k.cx / k.fx, t.inv22 = 1.0 / k.fy, t.inv23 = -k.cy / k.fy;
    for (int i = 0; i < 4; i++) t.poly[i] = k.poly[i];
    t.theta_lim = c.theta_lim, t.r_lim = c.r_lim;
    return t;
  }
  if (k.model == LFVIO_CAM_OCAM) {
    t.c = k.c, t.d = k.d, t.e = k.e;
    t.inv_scale = 1.0 / (k.c - k.d * k.e);
    for (int i = 0; i < 5; i++) t.poly[i] = k.poly[i];
    return t;
  }
  t.inv11 = 1.0 / k.fx, t.inv13 = -k.cx / k.fx, t.inv22 = 1.0 / k.fy, t.inv23 = -k.cy / k.fy;
  t.k1 = k.k1, t.k2 = k.k2, t.p1 = k.p1, t.p2 = k.p2;
  t.no_distortion = k.k1 == 0.0 && k.k2 == 0.0 && k.p1 == 0.0 && k.p2 == 0.0;
  if (k.model == LFVIO_CAM_MEI) t.xi = k.xi;
  return t;
}

// nullptr, or what is wrong with the camera or the point count
inline const char *track_common_check(const LfvioCamera *cam, int N) {
  if (!cam) return "lfvio_track: null camera";
  if (cam->model != LFVIO_CAM_OCAM && cam->model != LFVIO_CAM_PINHOLE && cam->model != LFVIO_CAM_MEI && cam->model != LFVIO_CAM_KANNALA_BRANDT)
    return "lfvio_track: a camera model other than LFVIO_CAM_OCAM, LFVIO_CAM_PINHOLE, LFVIO_CAM_MEI and LFVIO_CAM_KANNALA_BRANDT";
  if (cam->model == LFVIO_CAM_KANNALA_BRANDT) {
    const double v[8] = {cam->cx, cam->cy, cam->fx, cam->fy, cam->poly[0], cam->poly[1], cam->poly[2], cam->poly[3]};
    for (double x : v)
      if (!std::isfinite(x)) return "lfvio_track: a non-finite camera parameter";
    if (cam->fx == 0.0 || cam->fy == 0.0) return "lfvio_track: fx or fy is zero";
  } else if (cam->model != LFVIO_CAM_OCAM) {
    const double v[8] = {cam->cx, cam->cy, cam->fx, cam->fy, cam->k1, cam->k2, cam->p1, cam->p2};
    for (double x : v)
      if (!std::isfinite(x)) return "lfvio_track: a non-finite camera parameter";
    if (cam->fx == 0.0 || cam->fy == 0.0) return "lfvio_track: fx or fy is zero";
    if (cam->model == LFVIO_CAM_MEI && !std::isfinite(cam->xi)) return "lfvio_track: a non-finite xi";
  }
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
