// klt.inc — host side of lfvio_klt_track / lfvio_klt_reset / lfvio_klt_level (include/lfvio.h): the optical flow of
// FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:111-131) on the kernels of kernels_klt.h.  Included by
// lfvio_hip.hip inside its extern "C" block.
//
// One call: validate and plan (klt_plan.h), pack [points | image] into the staging block of feat.inc, one copy up, the image into the
// context's other pyramid buffer (a copy — k_img_gray of imgfmt.inc instead while lfvio_image_format_set names another encoding,
// k_remap_gray of tracksource.inc instead of both while lfvio_track_source_set is on — or
// the three CLAHE launches of clahe.inc while lfvio_clahe_set is on), k_klt_down per level,
// k_klt_track (grid N) from the resident pyramid into the new one, one copy down of [next | status | iterations]; then the new pyramid
// is the resident one.  The pyramid buffers are the context's own: the
// staging block is freed when it grows and overwritten by every feature call.

// levels from + 1 .. to of the pyramid at `pyr` (offsets and sizes of `full`, which covers every level of this image size)
static int klt_build(lfvio_ctx *c, hipStream_t fs, unsigned char *pyr, const KltPlan &full, int from, int to) {
  for (int k = from + 1; k <= to; k++) {
    hipLaunchKernelGGL(k_klt_down, dim3((full.w[k] + 63) / 64, (full.h[k] + 3) / 4), dim3(256), 0, fs, (const unsigned char *)(pyr + full.off[k - 1]),
                       full.w[k - 1], full.h[k - 1], pyr + full.off[k], full.w[k], full.h[k]);
    HIPCHK(c, hipGetLastError());
  }
  return LFVIO_OK;
}

// The image at d_image (device, W x H as `ti.im` describes it — or the source image `ti.src` describes, gathered through the resident
// map) into the context's other pyramid buffer — a copy, the conversion to grey or that gather, then CLAHE while it is on: in place
// behind a conversion or a gather, since clahe_map_body reads and writes the same pixel and nothing else and the histograms are a
// launch earlier — with the levels
// 1 .. LU, and the levels of the resident pyramid that an earlier call did not build.  *prev: the pyramid to track from (the new one
// when none of this size is resident, :111-114).  Returns the new pyramid, which the caller makes resident with a commit of the stream once the
// call has succeeded.  (Every earlier call on the feature stream has been waited for: nobody reads the other buffer.)
static int klt_pyramid(lfvio_ctx *c, hipStream_t fs, const unsigned char *d_image, const TrackImage &ti, int W, int H, const KltPlan &full, int LU,
                       const unsigned char **prev, unsigned char **fresh_out) {
  TrackStream &s = c->tstream;
  unsigned char *fresh = c->klt.d[1 - s.pcur], *resident = c->klt.d[s.pcur];
  const bool written = ti.source || ti.im.convert;  // level 0 is written by a kernel of its own; CLAHE, if on, reads it there
  if (ti.source) {  // d_image is the SOURCE image: level 0 is gathered through the resident map (tracksource.inc)
    if (int rc = tracksource_run(c, fs, ti.src, W, H, d_image, fresh)) return rc;
    d_image = fresh;
  } else if (ti.im.convert) {  // level 0 is the grey image
    if (int rc = imgfmt_run(c, fs, ti.im, W, H, d_image, fresh)) return rc;
    d_image = fresh;
  }
  if (c->clahe.on) {  // the equalized image is the image: k_clahe_map writes level 0 (clahe.inc)
    if (int rc = clahe_run(c, fs, c->clahe.cfg, W, H, d_image, fresh, nullptr)) return rc;
  } else if (!written) {
    HIPCHK(c, hipMemcpyAsync(fresh, d_image, (size_t)W * H, hipMemcpyDeviceToDevice, fs));
  }
  if (int rc = klt_build(c, fs, fresh, full, 0, LU)) return rc;
  if (s.levels_missing(W, H, LU)) {  // (an earlier call asked for fewer levels)
    if (int rc = klt_build(c, fs, resident, full, s.built, LU)) return rc;
    s.resident_built(LU);
  }
  *prev = s.resident(W, H) ? (const unsigned char *)resident : fresh, *fresh_out = fresh;  // otherwise the new image is both images (:111-114)
  return LFVIO_OK;
}
static KltArgs klt_args(const LfvioKltIn *in, const KltPlan &full, int LU) {
  KltArgs a;
  a.win = in->win_size, a.levels_used = LU, a.max_level = in->max_level, a.max_iter = in->max_iterations, a.border = in->border;
  a.eps2 = in->epsilon * in->epsilon, a.min_eig = in->min_eig_threshold;
  for (int l = 0; l < KLT_LEVELS; l++) a.w[l] = full.w[l], a.h[l] = full.h[l], a.off[l] = (long long)full.off[l];
  return a;
}

int lfvio_klt_track(lfvio_ctx *c, const LfvioKltIn *in, float *next_pts, unsigned char *status, int *iterations, LfvioKltOut *out) {
  if (!c || !in || !next_pts || !status || !out) return LFVIO_ERR_ARG;
  if (const char *why = klt_check(in)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int N = in->num_points, W = in->width, H = in->height, ML = in->max_level;
  TrackImage im;  // what goes up: the image, or under lfvio_track_source_set the source image
  if (const char *why = track_image_plan(c, W, H, &im)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const KltPlan p = klt_plan(W, H, in->win_size, ML), full = klt_plan(W, H, 0, LFVIO_KLT_MAX_LEVEL);
  const int LU = p.levels_used;
  FeatStage st(c);
  const size_t nI = im.bytes(), nT = (size_t)N * (ML + 1) * 4;
  const size_t oP = st.take((size_t)N * 8), oI = st.take(nI), in_end = st.end;
  const size_t oN = st.take((size_t)N * 8), oS = st.take((size_t)N), oT = st.take(nT);
  if (int rc = st.reserve()) return rc;
  // (every earlier call on the feature stream has been waited for: nobody reads the other buffer)
  if (!c->klt.d[1 - c->tstream.pcur].reserve(full.bytes)) return out_of_memory(c, "out of memory (image pyramid)");
  char *d = st.d, *h = st.h;
  if (N) std::memcpy(h + oP, in->prev_pts, (size_t)N * 8);
  std::memcpy(h + oI, in->image, nI);
  if (int rc = st.up(in_end)) return rc;
  unsigned char *fresh;
  const unsigned char *prev;
  if (int rc = klt_pyramid(c, st.fs, (const unsigned char *)(d + oI), im, W, H, full, LU, &prev, &fresh)) return rc;
  if (N) {
    hipLaunchKernelGGL(k_klt_track, dim3(N), dim3(KLT_THREADS), 0, st.fs, klt_args(in, full, LU), N, prev,
                       (const unsigned char *)fresh, (const float *)(d + oP), (float *)(d + oN), (unsigned char *)(d + oS),
                       iterations ? (int *)(d + oT) : (int *)nullptr);
    HIPCHK(c, hipGetLastError());
    if (int rc = st.down(oN, iterations ? st.end : oS + (size_t)N)) return rc;
  } else {
    HIPCHK(c, hipStreamSynchronize(st.fs));
  }
  int tracked = 0;
  if (N) {
    std::memcpy(next_pts, h + oN, (size_t)N * 8);
    std::memcpy(status, h + oS, (size_t)N);
    if (iterations) std::memcpy(iterations, h + oT, nT);
    for (int i = 0; i < N; i++) tracked += status[i] != 0;
  }
  out->levels_used = LU, out->num_tracked = tracked;
  c->tstream.commit_flow(W, H, LU);
  return LFVIO_OK;
}

int lfvio_klt_reset(lfvio_ctx *c) {
  if (!c) return LFVIO_ERR_ARG;
  c->tstream.reset_flow();
  return LFVIO_OK;
}

int lfvio_klt_level(lfvio_ctx *c, int level, int *width, int *height, unsigned char *pixels) {
  if (!c || !width || !height) return LFVIO_ERR_ARG;
  const TrackStream &k = c->tstream;
  if (!k.valid || level < 0 || level > k.built) {
    c->err = "lfvio_klt_level: no resident image, or a level that is not built";
    return LFVIO_ERR_ARG;
  }
  const KltPlan full = klt_plan(k.w, k.h, 0, LFVIO_KLT_MAX_LEVEL);
  if (pixels) {
    FeatStage st(c);
    HIPCHK(c, hipMemcpyAsync(pixels, c->klt.d[k.pcur] + full.off[level], (size_t)full.w[level] * full.h[level], hipMemcpyDeviceToHost, st.fs));
    HIPCHK(c, hipStreamSynchronize(st.fs));
  }
  *width = full.w[level], *height = full.h[level];
  return LFVIO_OK;
}
