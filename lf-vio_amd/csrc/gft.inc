// gft.inc — host side of lfvio_gft_detect / lfvio_gft_set_mask / lfvio_gft_response (include/lfvio.h): setMask and
// goodFeaturesToTrack of FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:46-83, :147-176) on the kernels of
// kernels_gft.h.  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate (gft_plan.h), pack [points | counts] into the staging block of feat.inc, one copy up, k_gft_thin, k_gft_response,
// k_gft_cand, the sort network, k_gft_pick, one copy down of [kept | corners | LfvioGftOut].  The image is level 0 of the resident
// pyramid of klt.inc and is only read.  The base mask and the work arrays (lambda, final mask, candidates) are device memory of the
// context's own, grow-only: no allocation once they have reached the image's size.

static int gft_reserve(lfvio_ctx *c, const GftWork &wk) {
  return c->gft.work.reserve(wk.bytes) ? LFVIO_OK : out_of_memory(c, "out of memory (corner detection)");
}

// img: level 0 of a pyramid of W x H — the resident one, or the one lfvio_track_frame is about to make resident
static int gft_launch_response(lfvio_ctx *c, hipStream_t fs, const GftWork &wk, const unsigned char *img, int W, int H, const unsigned char *base, int r,
                               int max_count) {
  char *w = c->gft.work;
  hipLaunchKernelGGL(k_gft_response, dim3((W + GFT_TX - 1) / GFT_TX, (H + GFT_TY - 1) / GFT_TY), dim3(GFT_THREADS), 0, fs, img, W, H, base,
                     (const int *)(w + wk.kxy), r, max_count, (GftDev *)(w + wk.st), (double *)(w + wk.lam), (unsigned char *)(w + wk.mask));
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

// Everything behind k_gft_thin: the response, the candidates, the sort network and the greedy pick into corners / *out (device).
static int gft_launch_detect(lfvio_ctx *c, hipStream_t fs, const GftWork &wk, const unsigned char *img, int W, int H, const unsigned char *base,
                             const LfvioGftIn *in, float *corners, LfvioGftOut *out) {
  char *w = c->gft.work;
  const int MC = in->max_count;
  GftDev *dev = (GftDev *)(w + wk.st);
  unsigned long long *ck = (unsigned long long *)(w + wk.keys);
  unsigned *ci = (unsigned *)(w + wk.idx);
  if (int rc = gft_launch_response(c, fs, wk, img, W, H, base, in->mask_radius, MC)) return rc;
  hipLaunchKernelGGL(k_gft_cand, dim3((W + GFT_THREADS - 1) / GFT_THREADS, (H + GFT_CAND_ROWS - 1) / GFT_CAND_ROWS), dim3(GFT_THREADS), 0, fs, (const double *)(w + wk.lam),
                     (const unsigned char *)(w + wk.mask), W, H, in->quality_level, MC, dev, ck, ci);
  HIPCHK(c, hipGetLastError());
  // the network of the arrays' capacity: the candidate count stays on the device, a stage beyond it returns at once (gft_plan.h)
  const GftSortGrid sg = gft_sort_grid(wk.capacity);
  gft_sort_stages(
      wk.capacity, [&](unsigned kk) { hipLaunchKernelGGL(k_gft_sort_local, dim3(sg.chunks), dim3(GFT_SORT_THREADS), 0, fs, (const GftDev *)dev, ck, ci, kk); },
      [&](unsigned kk, unsigned j) { hipLaunchKernelGGL(k_gft_sort_global, dim3(sg.halves), dim3(GFT_THREADS), 0, fs, (const GftDev *)dev, ck, ci, kk, j); });
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_gft_pick, dim3(1), dim3(GFT_THREADS), 0, fs, (const GftDev *)dev, (const unsigned *)ci, W, in->min_distance, MC, corners, out);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int lfvio_gft_detect(lfvio_ctx *c, const LfvioGftIn *in, int *kept, float *corners, LfvioGftOut *out) {
  if (!c || !in || !corners || !out) return LFVIO_ERR_ARG;
  if (const char *why = gft_check(in)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const TrackStream &k = c->tstream;
  lfvio_ctx::GftState &g = c->gft;
  const int N = in->num_points, MC = in->max_count;
  if ((N > 0 && !kept) || !k.valid || !k.mask_fits(k.w, k.h)) {
    c->err = "lfvio_gft_detect: null kept, no resident image, or a base mask that is not the resident image's size";
    return LFVIO_ERR_ARG;
  }
  const int W = k.w, H = k.h;
  const GftWork wk = gft_work(W, H);
  FeatStage st(c);
  const size_t oP = st.take((size_t)N * 8), oC = st.take((size_t)N * 4), in_end = st.end;
  const size_t oK = st.take((size_t)N * 4), oX = st.take((size_t)MC * 8), oO = st.take(sizeof(LfvioGftOut));
  if (int rc = st.reserve()) return rc;
  if (int rc = gft_reserve(c, wk)) return rc;
  char *d = st.d, *h = st.h, *w = g.work;
  if (N) {
    std::memcpy(h + oP, in->pts, (size_t)N * 8);
    std::memcpy(h + oC, in->track_cnt, (size_t)N * 4);
    if (int rc = st.up(in_end)) return rc;
  }
  const unsigned char *base = k.mask_set ? g.mask : nullptr;
  hipLaunchKernelGGL(k_gft_thin<int>, dim3(1), dim3(GFT_THREADS), 0, st.fs, N, (const float *)(d + oP), (const int *)(d + oC), base, W, H, in->mask_radius,
                     (GftDev *)(w + wk.st), (int *)(d + oK), (int *)(w + wk.kxy));
  HIPCHK(c, hipGetLastError());
  if (int rc = gft_launch_detect(c, st.fs, wk, c->klt.d[k.pcur], W, H, base, in, (float *)(d + oX), (LfvioGftOut *)(d + oO))) return rc;
  if (int rc = st.down(oK, st.end)) return rc;
  LfvioGftOut o;
  std::memcpy(&o, h + oO, sizeof o);
  if (o.num_kept) std::memcpy(kept, h + oK, (size_t)o.num_kept * 4);
  if (o.num_corners) std::memcpy(corners, h + oX, (size_t)o.num_corners * 8);
  *out = o;
  return LFVIO_OK;
}

int lfvio_gft_set_mask(lfvio_ctx *c, int width, int height, const unsigned char *pixels) {
  if (!c) return LFVIO_ERR_ARG;
  lfvio_ctx::GftState &g = c->gft;
  if (!pixels) {
    c->tstream.mask_cleared();
    return LFVIO_OK;
  }
  if (const char *why = gft_mask_check(width, height, c->tstream.resident_w(), c->tstream.h)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const size_t n = (size_t)width * height;
  FeatStage st(c);
  const size_t oM = st.take(n);
  if (int rc = st.reserve()) return rc;
  if (g.mask.capacity() < n) {  // the new block first: a failure leaves the old mask, and mask_set, as they are
    DevBuf<unsigned char> fresh;
    if (!fresh.reserve(n)) return out_of_memory(c, "out of memory (base mask)");
    HIPCHK(c, hipStreamSynchronize(st.fs));
    g.mask = std::move(fresh), c->tstream.mask_cleared();
  }
  std::memcpy(st.h + oM, pixels, n);
  if (int rc = st.up(st.end)) return rc;
  HIPCHK(c, hipMemcpyAsync(g.mask, st.d + oM, n, hipMemcpyDeviceToDevice, st.fs));
  HIPCHK(c, hipStreamSynchronize(st.fs));
  c->tstream.mask_is(width, height);
  return LFVIO_OK;
}

int lfvio_gft_response(lfvio_ctx *c, double *response) {
  if (!c || !response) return LFVIO_ERR_ARG;
  const TrackStream &k = c->tstream;
  if (!k.valid) {
    c->err = "lfvio_gft_response: no resident image";
    return LFVIO_ERR_ARG;
  }
  const GftWork wk = gft_work(k.w, k.h);
  FeatStage st(c);
  if (int rc = gft_reserve(c, wk)) return rc;
  HIPCHK(c, hipMemsetAsync(c->gft.work + wk.st, 0, sizeof(GftDev), st.fs));  // no kept points
  if (int rc = gft_launch_response(c, st.fs, wk, c->klt.d[k.pcur], k.w, k.h, nullptr, 0, 1)) return rc;
  HIPCHK(c, hipMemcpyAsync(response, c->gft.work + wk.lam, (size_t)k.w * k.h * 8, hipMemcpyDeviceToHost, st.fs));
  HIPCHK(c, hipStreamSynchronize(st.fs));
  return LFVIO_OK;
}
