// track.inc — host side of lfvio_track_reject / lfvio_track_undistort / lfvio_track_reset (include/lfvio.h): rejectWithF and
// undistortedPoints of FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:329-386, :441-504) on the kernels of
// kernels_track.h and k_tv_hyp of kernels_twoview.h.  Included by lfvio_hip.hip inside its extern "C" block.
//
// lfvio_track_reject: validate (track_plan.h), pack [cur_pts | forw_pts | samples] into the staging block of feat.inc (16 bytes a
// match, where lfvio_two_view takes 48), one copy up, k_trk_lift, k_tv_hyp (grid S), k_trk_fit (one workgroup), one copy down of
// [LfvioTrackRejectOut | status | bearings] as far as the caller asked.
// lfvio_track_undistort: [pts | ids] up, k_trk_undist, [un_pts | un_pts_3d | velocity_3d | matched] down.  The (id, un_pts_3d) pairs
// live in two buffers of the context's own; the kernel reads the stream's `mcur` and writes the other, and the host swaps them when the call has
// succeeded: a refused or failed call leaves the resident map and time as they were.

int lfvio_track_reject(lfvio_ctx *c, const LfvioTrackRejectIn *in, unsigned char *status, LfvioTrackRejectOut *out, double *bearing_cur,
                       double *bearing_forw) {
  if (!c || !in || !status || !out) return LFVIO_ERR_ARG;
  if (const char *why = track_reject_check(in)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int N = in->num_points, S = in->num_samples;
  if (N < TRACK_MIN_MATCHES) {  // :331
    if (N) std::memset(status, 1, (size_t)N);
    out->status = 2, out->best_sample = -1, out->num_inliers = 0, out->best_score = 0.0;
    return LFVIO_OK;
  }
  const TrackCam cam = track_cam(*in->camera, &c->track_kb);
  FeatStage st(c);
  const size_t NR = (size_t)std::max(N, 9);
  const size_t oP = st.take((size_t)N * 8), oQ = st.take((size_t)N * 8), oS = st.take((size_t)S * 32), in_end = st.end;
  const size_t oA = st.take(NR * 72), oC = st.take((size_t)S * 4), oE = st.take((size_t)S * 72);
  const size_t oO = st.take(sizeof(LfvioTrackRejectOut)), oM = st.take((size_t)N), oL = st.take((size_t)N * 24), oR = st.take((size_t)N * 24);
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oP, in->cur_pts, (size_t)N * 8);
  std::memcpy(h + oQ, in->forw_pts, (size_t)N * 8);
  std::memcpy(h + oS, in->samples, (size_t)S * 32);
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_trk_lift, dim3((2 * N + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, st.fs, cam, N, (const float *)(d + oP),
                     (const float *)(d + oQ), (double *)(d + oL), (double *)(d + oR));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_tv_hyp, dim3(S), dim3(TV_HYP_THREADS), 0, st.fs, N, (const double *)(d + oL), (const double *)(d + oR),
                     (const int *)(d + oS), (double *)(d + oE), (float *)(d + oC));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_trk_fit, dim3(1), dim3(TV_FIT_THREADS), 0, st.fs, N, S, (const double *)(d + oL), (const double *)(d + oR),
                     (const double *)(d + oE), (const float *)(d + oC), (double *)(d + oA), (unsigned char *)(d + oM),
                     (LfvioTrackRejectOut *)(d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, bearing_cur || bearing_forw ? st.end : oM + (size_t)N)) return rc;
  track_reject_copy(out, *(const LfvioTrackRejectOut *)(h + oO));  // no model: E stays as the caller had it
  std::memcpy(status, h + oM, (size_t)N);
  if (bearing_cur) std::memcpy(bearing_cur, h + oL, (size_t)N * 24);
  if (bearing_forw) std::memcpy(bearing_forw, h + oR, (size_t)N * 24);
  return LFVIO_OK;
}

int lfvio_track_undistort(lfvio_ctx *c, const LfvioTrackUndistortIn *in, float *un_pts, float *un_pts_3d, float *velocity_3d, int *matched) {
  if (!c || !in) return LFVIO_ERR_ARG;
  if (const char *why = track_undistort_check(in)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int N = in->num_points;
  if (N > 0 && (!un_pts || !un_pts_3d || !velocity_3d)) {
    c->err = "lfvio_track_undistort: null outputs";
    return LFVIO_ERR_ARG;
  }
  TrackStream &t = c->tstream;
  if (N == 0) {  // an empty map (:462): the next call's velocities are all 0
    t.commit_undistort(0, in->time);
    return LFVIO_OK;
  }
  const TrackCam cam = track_cam(*in->camera, &c->track_kb);
  FeatStage st(c);
  const size_t oP = st.take((size_t)N * 8), oI = st.take((size_t)N * 4), in_end = st.end;
  const size_t oU = st.take((size_t)N * 8), o3 = st.take((size_t)N * 12), oV = st.take((size_t)N * 12), oM = st.take((size_t)N * 4);
  if (int rc = st.reserve()) return rc;
  for (auto &m : c->track.map)
    if (!m.reserve(TRACK_MAP_BYTES)) return out_of_memory(c, "out of memory (track map)");
  char *d = st.d, *h = st.h;
  std::memcpy(h + oP, in->pts, (size_t)N * 8);
  std::memcpy(h + oI, in->ids, (size_t)N * 4);
  if (int rc = st.up(in_end)) return rc;
  const char *prev = c->track.map[t.mcur];
  char *next = c->track.map[1 - t.mcur];
  hipLaunchKernelGGL(k_trk_undist, dim3((N + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, st.fs, cam, N, (const float *)(d + oP),
                     (const int *)(d + oI), in->time - t.time, t.mcount, (const int *)prev, (const float *)(prev + TRACK_MAP_IDS), (float *)(d + oU),
                     (float *)(d + o3), (float *)(d + oV), (int *)(d + oM), (int *)next, (float *)(next + TRACK_MAP_IDS));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oU, st.end)) return rc;
  std::memcpy(un_pts, h + oU, (size_t)N * 8);
  std::memcpy(un_pts_3d, h + o3, (size_t)N * 12);
  std::memcpy(velocity_3d, h + oV, (size_t)N * 12);
  if (matched) std::memcpy(matched, h + oM, (size_t)N * 4);
  t.commit_undistort(N, in->time);
  return LFVIO_OK;
}

int lfvio_track_reset(lfvio_ctx *c) {
  if (!c) return LFVIO_ERR_ARG;
  c->tstream.reset_map();
  return LFVIO_OK;
}
