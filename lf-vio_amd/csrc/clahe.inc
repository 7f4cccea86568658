// clahe.inc — host side of lfvio_clahe_set / lfvio_clahe_apply (include/lfvio.h) and of the equalize step of lfvio_klt_track
// (klt.inc): cv::createCLAHE(...)->apply of FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:101-107) on the kernels
// of kernels_clahe.h.  Included by lfvio_hip.hip inside its extern "C" block, in front of klt.inc.
//
// clahe_run is the three launches: histograms of `src` into the context's int table, the LUTs, the map from `src` to `dst`.  In
// lfvio_klt_track `dst` is level 0 of the fresh pyramid buffer and the LUTs are the context's; in lfvio_clahe_apply both are segments
// of the staging block of feat.inc and come down in one copy.  The table and the LUTs are device memory of the context's own, sized
// once for LFVIO_CLAHE_MAX_TILES^2 tiles (320 KiB); k_clahe_lut leaves the table zero.

constexpr size_t CLAHE_TABLE_BYTES = (size_t)LFVIO_CLAHE_MAX_TILES * LFVIO_CLAHE_MAX_TILES * 256 * sizeof(int);
constexpr size_t CLAHE_LUT_BYTES = (size_t)LFVIO_CLAHE_MAX_TILES * LFVIO_CLAHE_MAX_TILES * 256;

static int clahe_reserve(lfvio_ctx *c, hipStream_t fs) {
  lfvio_ctx::ClaheState &s = c->clahe;
  if (!s.work) {
    if (!s.work.reserve(CLAHE_TABLE_BYTES + CLAHE_LUT_BYTES)) return out_of_memory(c, "out of memory (CLAHE)");
    s.dirty = true;
  }
  if (s.dirty) {  // fresh memory, or a call that failed between the histograms and the LUTs
    HIPCHK(c, hipMemsetAsync(s.work, 0, CLAHE_TABLE_BYTES, fs));
    s.dirty = false;
  }
  return LFVIO_OK;
}

// src -> dst (both W x H, 4-aligned) on fs; lut: where the [tiles_y][tiles_x][256] bytes go (nullptr: the context's own)
static int clahe_run(lfvio_ctx *c, hipStream_t fs, const LfvioClaheIn &cfg, int W, int H, const unsigned char *src, unsigned char *dst, unsigned char *lut) {
  if (int rc = clahe_reserve(c, fs)) return rc;
  lfvio_ctx::ClaheState &s = c->clahe;
  const ClahePlan p = clahe_plan(W, H, cfg);
  const int tiles = cfg.tiles_x * cfg.tiles_y, bands = (p.th + CLAHE_BAND_ROWS - 1) / CLAHE_BAND_ROWS;
  int *table = (int *)s.work.get();
  if (!lut) lut = (unsigned char *)s.work.get() + CLAHE_TABLE_BYTES;
  s.dirty = true;
  hipLaunchKernelGGL(k_clahe_hist, dim3(tiles, bands), dim3(CLAHE_THREADS), 0, fs, src, W, H, cfg.tiles_x, p.tw, p.th, table);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_clahe_lut, dim3(tiles), dim3(CLAHE_THREADS), 0, fs, table, p.clip, p.lut_scale, lut);
  HIPCHK(c, hipGetLastError());
  s.dirty = false;
  const dim3 grid((W + CLAHE_MAP_COLS - 1) / CLAHE_MAP_COLS, (cfg.tiles_y + 1) * bands);
  if (W % 4 == 0)
    hipLaunchKernelGGL(k_clahe_map<true>, grid, dim3(CLAHE_THREADS), 0, fs, src, dst, W, H, cfg.tiles_x, cfg.tiles_y, p.th, bands, p.inv_tw, p.inv_th,
                       (const unsigned char *)lut);
  else
    hipLaunchKernelGGL(k_clahe_map<false>, grid, dim3(CLAHE_THREADS), 0, fs, src, dst, W, H, cfg.tiles_x, cfg.tiles_y, p.th, bands, p.inv_tw, p.inv_th,
                       (const unsigned char *)lut);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int lfvio_clahe_set(lfvio_ctx *c, const LfvioClaheIn *cfg) {
  if (!c) return LFVIO_ERR_ARG;
  if (!cfg) {
    c->clahe.on = false;
    return LFVIO_OK;
  }
  if (const char *why = clahe_check(cfg)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  c->clahe.cfg = *cfg, c->clahe.on = true;
  return LFVIO_OK;
}

int lfvio_clahe_apply(lfvio_ctx *c, const LfvioClaheIn *cfg, int width, int height, const unsigned char *pixels, unsigned char *out, unsigned char *lut) {
  if (!c || !cfg || !pixels || !out) return LFVIO_ERR_ARG;
  const char *why = clahe_check(cfg);
  if (!why) why = clahe_size_check(width, height);
  if (why) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const size_t nI = (size_t)width * height, nL = (size_t)cfg->tiles_x * cfg->tiles_y * 256;
  FeatStage st(c);
  const size_t oI = st.take(nI), in_end = st.end, oO = st.take(nI), oL = st.take(nL);
  if (int rc = st.reserve()) return rc;
  std::memcpy(st.h + oI, pixels, nI);
  if (int rc = st.up(in_end)) return rc;
  if (int rc = clahe_run(c, st.fs, *cfg, width, height, (const unsigned char *)(st.d + oI), (unsigned char *)(st.d + oO), (unsigned char *)(st.d + oL))) return rc;
  if (int rc = st.down(oO, st.end)) return rc;
  std::memcpy(out, st.h + oO, nI);
  if (lut) std::memcpy(lut, st.h + oL, nL);
  return LFVIO_OK;
}
