// trackframe.inc — host side of lfvio_track_frame / lfvio_track_frame_reset (include/lfvio.h): one image through
// FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:95-184) and updateID (feature_tracker_node.cpp:102-111) as ONE
// upload, the launches of klt.inc, track.inc and gft.inc back to back with the kernels of kernels_trackframe.h between them, and
// ONE download.  Included by lfvio_hip.hip inside its extern "C" block.
//
// The host knows only bounds: n0, the table's count, for n1 and n2, and B = max(n0, max_count) for the count after the call (n0
// without publish).  Every grid and every segment of the staging block is sized for its bound; the kernels read the true count from
// the TfDev at the head of the block that comes down, and the host reads it there afterwards.  The table, the pyramid and the
// (id, un_pts_3d) map are each written into the context's OTHER buffer and swapped at the end (TrackStream::commit_frame): a call that
// is refused or fails leaves all three, n_id and the time as they were.

// lfvio_track_frame (msg null) and lfvio_track_frame_message: with a message and publish the rows are one more segment of the block
// that comes down (trackframe_message_bytes), written by k_tf_message behind k_trk_undist_n.
static int track_frame_run(lfvio_ctx *c, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, const LfvioTrackFrameStages *stages, LfvioTrackMessage *msg) {
  if (!c || !in || !out) return LFVIO_ERR_ARG;
  TrackStream &s = c->tstream;
  lfvio_ctx::TrackFrameState &f = c->tframe;
  lfvio_ctx::TrackState &t = c->track;
  lfvio_ctx::GftState &g = c->gft;
  if (const char *why = trackframe_check(in, s.count)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int W = in->width, H = in->height, S = in->num_samples, MC = in->max_count, n0 = s.count;
  TrackImage im;  // what goes up: the image, or under lfvio_track_source_set the source image
  if (const char *why = track_image_plan(c, W, H, &im)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const bool pub = in->publish != 0;
  if (!trackframe_out_check(out, nullptr) || (pub && !s.mask_fits(W, H))) {  // (a message's rows: lfvio_track_frame_message's check)
    c->err = "lfvio_track_frame: a null array in out, or a base mask that is not the image's size";
    return LFVIO_ERR_ARG;
  }
  const LfvioKltIn kin = trackframe_klt(in);
  const LfvioGftIn gin = trackframe_gft(in);
  const KltPlan full = klt_plan(W, H, 0, LFVIO_KLT_MAX_LEVEL);
  const int LU = klt_plan(W, H, in->win_size, in->max_level).levels_used;
  const TrackCam cam = track_cam(*in->camera, &c->track_kb);
  const GftWork wk = gft_work(W, H);
  const size_t B = (size_t)trackframe_bound(n0, MC, pub), N0 = (size_t)n0, nI = im.bytes();
  FeatStage st(c);
  // up
  const size_t oW = st.take(pub ? (size_t)S * 32 : 0), oI = st.take(nI), in_end = st.end;
  // between the stages
  const size_t oC1 = st.take(N0 * 8), oT1 = st.take(N0 * 16), oT2 = st.take(N0 * 16), oL = st.take(N0 * 24), oR = st.take(N0 * 24);
  const size_t oA = st.take(std::max<size_t>(N0, 9) * 72), oSc = st.take((size_t)S * 4), oE = st.take((size_t)S * 72);
  const size_t oRaw = st.take(B * 4), oMt = st.take(B * 4);
  // down: the counts and records, the table, the outputs of undistortedPoints; the stages behind them, for a caller who asks
  const size_t oD = st.take(sizeof(TfDev)), oTab = st.take(B * 16), oU = st.take(B * 8), o3 = st.take(B * 12), oV = st.take(B * 12);
  const bool rows = msg && pub;
  const size_t oMsg = rows ? st.take(trackframe_message_bytes(B)) : 0, main_end = st.end;
  const size_t oN = st.take(N0 * 8), oSt = st.take(N0), oSm = st.take((size_t)S * 32), oM = st.take(N0), oK = st.take(N0 * 4), oX = st.take((size_t)MC * 8);
  if (int rc = st.reserve()) return rc;
  if (pub)
    if (int rc = gft_reserve(c, wk)) return rc;
  if (!c->klt.d[1 - s.pcur].reserve(full.bytes)) return out_of_memory(c, "out of memory (image pyramid)");
  for (auto &b : f.table)
    if (!b.reserve(TRACK_TABLE_BYTES)) return out_of_memory(c, "out of memory (track table)");
  for (auto &m : t.map)
    if (!m.reserve(TRACK_MAP_BYTES)) return out_of_memory(c, "out of memory (track map)");
  char *d = st.d, *h = st.h;
  if (pub) std::memcpy(h + oW, in->sample_words, (size_t)S * 32);
  std::memcpy(h + oI, in->image, nI);
  if (int rc = st.up(in_end)) return rc;

  TfDev *dev = (TfDev *)(d + oD);
  const TfTable have = tf_table(f.table[s.tcur], LFVIO_TRACK_MAX_POINTS), next = tf_table(f.table[1 - s.tcur], LFVIO_TRACK_MAX_POINTS);
  const TfTable t1 = tf_table(d + oT1, N0), t2 = tf_table(d + oT2, N0), down = tf_table(d + oTab, B);
  // 1: the flow
  unsigned char *fresh;
  const unsigned char *prev;
  if (int rc = klt_pyramid(c, st.fs, (const unsigned char *)(d + oI), im, W, H, full, LU, &prev, &fresh)) return rc;
  if (n0) {
    hipLaunchKernelGGL(k_klt_track, dim3(n0), dim3(KLT_THREADS), 0, st.fs, klt_args(&kin, full, LU), n0, prev, (const unsigned char *)fresh,
                       (const float *)have.pts, (float *)(d + oN), (unsigned char *)(d + oSt), (int *)nullptr);
    HIPCHK(c, hipGetLastError());
  }
  // 2: reduceVector, track_cnt++, the sample sets
  hipLaunchKernelGGL(k_tf_flow, dim3(1), dim3(TF_THREADS), 0, st.fs, n0, (const unsigned char *)(d + oSt), (const float *)have.pts, (const float *)(d + oN),
                     (const int *)have.ids, (const int *)have.cnt, (float *)(d + oC1), t1, dev, S, pub ? (const unsigned *)(d + oW) : (const unsigned *)nullptr,
                     (int *)(d + oSm));
  HIPCHK(c, hipGetLastError());
  if (pub) {
    // 3: rejectWithF on n1 matches, reduceVector by its mask
    if (n0 >= TRACK_MIN_MATCHES) {  // (n1 <= n0: below 8 neither kernel would do anything)
      hipLaunchKernelGGL(k_trk_lift_n, dim3((2 * n0 + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, st.fs, cam, (const int *)&dev->n1,
                         (const float *)(d + oC1), (const float *)t1.pts, (double *)(d + oL), (double *)(d + oR));
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_tv_hyp_n, dim3(S), dim3(TV_HYP_THREADS), 0, st.fs, (const int *)&dev->n1, (const double *)(d + oL), (const double *)(d + oR),
                         (const int *)(d + oSm), (double *)(d + oE), (float *)(d + oSc));
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_trk_fit_n, dim3(1), dim3(TV_FIT_THREADS), 0, st.fs, (const int *)&dev->n1, S, (const double *)(d + oL), (const double *)(d + oR),
                       (const double *)(d + oE), (const float *)(d + oSc), (double *)(d + oA), (unsigned char *)(d + oM), &dev->reject);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_tf_reject, dim3(1), dim3(TF_THREADS), 0, st.fs, (const unsigned char *)(d + oM), t1, t2, dev);
    HIPCHK(c, hipGetLastError());
    // 4: setMask and goodFeaturesToTrack on the new image
    const unsigned char *base = s.mask_set ? (const unsigned char *)g.mask : nullptr;
    hipLaunchKernelGGL(k_gft_thin<const int *>, dim3(1), dim3(GFT_THREADS), 0, st.fs, (const int *)&dev->n2, (const float *)t2.pts, (const int *)t2.cnt, base, W, H,
                       gin.mask_radius, (GftDev *)(g.work + wk.st), (int *)(d + oK), (int *)(g.work + wk.kxy));
    HIPCHK(c, hipGetLastError());
    if (int rc = gft_launch_detect(c, st.fs, wk, fresh, W, H, base, &gin, (float *)(d + oX), &dev->detect)) return rc;
  }
  // 4 and 6: the next table, numbered; ids_raw keeps the -1 for step 5
  hipLaunchKernelGGL(k_tf_finish, dim3(1), dim3(TF_THREADS), 0, st.fs, pub ? 1 : 0, pub ? t2 : t1, (const int *)(d + oK), (const float *)(d + oX), s.n_id, next,
                     down, (int *)(d + oRaw), dev);
  HIPCHK(c, hipGetLastError());
  // 5: undistortedPoints
  if (B) {
    const char *pm = t.map[s.mcur];
    char *nm = t.map[1 - s.mcur];
    hipLaunchKernelGGL(k_trk_undist_n, dim3((unsigned)((B + TRK_THREADS - 1) / TRK_THREADS)), dim3(TRK_THREADS), 0, st.fs, cam, (const int *)&dev->num_points,
                       (const float *)down.pts, (const int *)(d + oRaw), in->time - s.time, s.mcount, (const int *)pm, (const float *)(pm + TRACK_MAP_IDS),
                       (float *)(d + oU), (float *)(d + o3), (float *)(d + oV), (int *)(d + oMt), (int *)nm, (float *)(nm + TRACK_MAP_IDS));
    HIPCHK(c, hipGetLastError());
  }
  if (rows) {
    hipLaunchKernelGGL(k_tf_message, dim3(1), dim3(TF_THREADS), 0, st.fs, (const TfDev *)dev, (int)B, down, (const float *)(d + o3), (const float *)(d + oV),
                       (int *)(d + oMsg), (float *)(d + oMsg + TF_MSG_HEAD));
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.down(oD, stages ? st.end : main_end)) return rc;

  const TfDev *o = (const TfDev *)(h + oD);
  if (!trackframe_counts_check(*o, n0, MC, pub, rows ? *(const int *)(h + oMsg) : 0)) {
    c->err = "lfvio_track_frame: a count from the device beyond its bound";
    return LFVIO_ERR_DEVICE;
  }
  trackframe_emit(TfDown{o, h + oTab, B, h + oU, h + o3, h + oV, rows ? h + oMsg : nullptr}, LU, pub, out, msg);
  if (stages) {
    if (stages->next_pts) std::memcpy(stages->next_pts, h + oN, N0 * 8);
    if (stages->status) std::memcpy(stages->status, h + oSt, N0);
    if (pub) {
      if (stages->samples && o->n1 >= TRACK_MIN_MATCHES) std::memcpy(stages->samples, h + oSm, (size_t)S * 32);
      if (stages->mask) std::memcpy(stages->mask, h + oM, (size_t)o->n1);
      if (stages->kept) std::memcpy(stages->kept, h + oK, (size_t)o->detect.num_kept * 4);
      if (stages->corners) std::memcpy(stages->corners, h + oX, (size_t)o->detect.num_corners * 8);
    }
  }
  s.commit_frame(W, H, LU, o->num_points, o->num_new, in->time);
  return LFVIO_OK;
}

int lfvio_track_frame(lfvio_ctx *c, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, const LfvioTrackFrameStages *stages) {
  return track_frame_run(c, in, out, stages, nullptr);
}

int lfvio_track_frame_message(lfvio_ctx *c, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, const LfvioTrackFrameStages *stages, LfvioTrackMessage *msg) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = trackframe_message_check(msg)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  return track_frame_run(c, in, out, stages, msg);
}

int lfvio_track_frame_reset(lfvio_ctx *c) {
  if (!c) return LFVIO_ERR_ARG;
  c->tstream.reset_frame();
  return LFVIO_OK;
}
