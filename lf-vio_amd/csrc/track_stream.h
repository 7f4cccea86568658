// track_stream.h — the scalars of ONE image stream of the tracker, and the moves the host makes on them.  The single route
// (lfvio_klt_track, lfvio_gft_*, lfvio_track_*, lfvio_track_frame) keeps one TrackStream in the context beside its buffers; every slot
// of the batched route (lfvio_track_batch_*) is one.  The buffers themselves are not here: a stream says WHICH of two is the resident
// one and what it holds.  Plain C++ (no HIP): klt.inc, gft.inc, track.inc, trackframe.inc and trackbatch.inc use it,
// tests/test_track_stream.py compiles it alone with g++ and holds every move to a restatement.
//
// Every double buffer follows one rule: a call writes the OTHER buffer and the commit makes it the resident one, so a call that is
// refused or fails leaves the stream as it was.
#pragma once

struct TrackStream {
  int pcur = 0, w = 0, h = 0, built = 0;  // the pyramid: buffer pcur holds levels 0 .. built of a w x h image
  bool valid = false;                     //   ... if any image is resident at all
  int mw = 0, mh = 0;                     // the base mask's size
  bool mask_set = false;                  //   ... if one is set (none: all 255)
  int tcur = 0, count = 0, n_id = 0;      // the track table: buffer tcur holds `count` entries; n_id is the next id to hand out
  int mcur = 0, mcount = 0;               // the (id, un_pts_3d) map: buffer mcur holds the `mcount` pairs of the previous call
  double time = 0.0;                      //   ... and that call's time

  // ---- the pyramid
  // a pyramid of W x H is resident: the flow tracks from it.  Otherwise the new image is both images (feature_tracker.cpp:111-114)
  bool resident(int W, int H) const { return valid && w == W && h == H; }
  // levels above 0 that the pyramid a call tracks from holds: the resident one's, or all LU of the fresh one
  int prev_built(int W, int H, int LU) const { return resident(W, H) ? built : LU; }
  // levels still to build on the resident pyramid for a call that uses LU (an earlier call asked for fewer: a level is a function
  // of the one below); they are built + 1 .. LU
  int levels_missing(int W, int H, int LU) const { return LU > prev_built(W, H, LU) ? LU - prev_built(W, H, LU) : 0; }
  // ... and they have been enqueued
  void resident_built(int LU) { built = LU; }
  // the width gft_mask_check takes for "the resident image" (0: none)
  int resident_w() const { return valid ? w : 0; }

  // ---- the base mask
  bool mask_fits(int W, int H) const { return !mask_set || (mw == W && mh == H); }
  void mask_is(int W, int H) { mw = W, mh = H, mask_set = true; }
  void mask_cleared() { mask_set = false; }

  // ---- the commits, each once its call has succeeded
  // a flow call: the other pyramid buffer, with levels 0 .. LU of a W x H image, is the resident one
  void commit_flow(int W, int H, int LU) { pcur = 1 - pcur, w = W, h = H, built = LU, valid = true; }
  // an undistort call over N points.  N = 0 wrote nothing: an empty map, the next call's velocities are all 0 (:462)
  void commit_undistort(int N, double t) {
    if (N) mcur = 1 - mcur;
    mcount = N, time = t;
  }
  // a frame: the table and the pyramid always swap, the map as an undistort call over num_points
  void commit_frame(int W, int H, int LU, int num_points, int num_new, double t) {
    commit_flow(W, H, LU);
    commit_undistort(num_points, t);
    tcur = 1 - tcur, count = num_points, n_id += num_new;
  }

  // ---- the resets.  None of them touches the base mask, and none a buffer index: what a buffer holds is simply forgotten.
  void reset_flow() { valid = false; }       // lfvio_klt_reset
  void reset_map() { mcount = 0, time = 0.0; }  // lfvio_track_reset
  void reset_frame() {                       // lfvio_track_frame_reset, lfvio_track_batch_reset
    reset_flow(), reset_map();
    count = 0, n_id = 0;
  }
};
