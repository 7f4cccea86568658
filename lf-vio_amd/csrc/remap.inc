// remap.inc — host side of lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply / lfvio_remap_reset (include/lfvio.h, DESIGN.md
// 3w) on the kernels of kernels_remap.h: spaceToPlane of the four camera models, the map of pointcloud_image_fusion's GetremapMat and
// of OCAMCamera::initUndistortRectifyMap, and cv::remap(..., INTER_NEAREST) through it.  Included by lfvio_hip.hip inside its extern
// "C" block, behind imgfmt.inc.
//
// Every check is remap_plan.h's and runs before anything is touched.  The float maps and the integer map are device memory of the
// context's own (lfvio_ctx::RemapState, allocated at the first build, grown for a larger output); points, images and the gathered
// output travel through the staging block of feat.inc.  All four calls run on the feature stream and leave the tracker's state alone.

int lfvio_cam_project(lfvio_ctx *c, const LfvioProjector *proj, int n, const double *P, double *px) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = remap_project_check(proj, n, P, px)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  if (n == 0) return LFVIO_OK;
  const ProjCam cam = proj_cam(*proj, &c->remap.kb);
  const size_t nI = (size_t)n * 3 * sizeof(double), nO = (size_t)n * 2 * sizeof(double);
  FeatStage st(c);
  const size_t oI = st.take(nI), in_end = st.end, oO = st.take(nO);
  if (int rc = st.reserve()) return rc;
  std::memcpy(st.h + oI, P, nI);
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_cam_project, dim3(remap_project_blocks(n)), dim3(REMAP_PROJECT_THREADS), 0, st.fs, cam, n, (const double *)(st.d + oI), (double *)(st.d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, st.end)) return rc;
  std::memcpy(px, st.h + oO, nO);
  return LFVIO_OK;
}

int lfvio_remap_build(lfvio_ctx *c, const LfvioRemapIn *in, float *map_x, float *map_y) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = remap_build_check(in, map_x, map_y)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  lfvio_ctx::RemapState &s = c->remap;
  RemapBuildArgs a = {};
  a.cam = proj_cam(*in->proj, &s.kb);
  a.kind = in->kind, a.width = in->width, a.height = in->height;
  for (int k = 0; k < 9; k++) a.M[k] = in->kind == LFVIO_MAP_PERSPECTIVE ? in->M[k] : 0.0;
  a.g = s.r.geom;  // of the last apply (bpp 0: there was none): a steady stream's integer map is written here, once
  const size_t n = (size_t)in->width * in->height;
  FeatStage st(c);
  s.r.valid = s.r.indexed = false;  // until the new maps are enqueued: a failure below leaves no map, not a stale one
  if (!s.map.reserve(2 * n * sizeof(float)) || !s.index.reserve(n * sizeof(int))) return out_of_memory(c, "out of memory (remap maps)");
  float *mx = s.map.get(), *my = mx + n;
  const RemapGrid g = remap_build_grid(in->width, in->height);
  hipLaunchKernelGGL(k_remap_build, dim3(g.x, g.y), dim3(REMAP_THREADS), 0, st.fs, a, mx, my, s.index.get());
  HIPCHK(c, hipGetLastError());
  if (map_x) {
    HIPCHK(c, hipMemcpyAsync(map_x, mx, n * sizeof(float), hipMemcpyDeviceToHost, st.fs));
    HIPCHK(c, hipMemcpyAsync(map_y, my, n * sizeof(float), hipMemcpyDeviceToHost, st.fs));
    HIPCHK(c, hipStreamSynchronize(st.fs));
  }
  s.r.valid = true, s.r.width = in->width, s.r.height = in->height, s.r.indexed = a.g.bpp != 0;
  return LFVIO_OK;
}

// The integer map of the RESIDENT maps (valid: the caller's check) made the one of a source of geometry g, on fs: rebuilt from the
// float maps where remap_needs_index says so, and only there.  Everyone who reads the integer map — remap_gather below and the
// tracker calls under lfvio_track_source_set (tracksource.inc) — comes through here first, so whoever finds it written for another
// geometry rebuilds it and the one RemapResident says whose it is.
static int remap_index_for(lfvio_ctx *c, hipStream_t fs, const RemapGeom &g) {
  lfvio_ctx::RemapState &s = c->remap;
  if (!remap_needs_index(s.r, g)) return LFVIO_OK;
  const size_t n = (size_t)s.r.width * s.r.height;
  const float *mx = s.map.get(), *my = mx + n;
  s.r.indexed = false;
  hipLaunchKernelGGL(k_remap_index, dim3((unsigned)((n + REMAP_THREADS - 1) / REMAP_THREADS)), dim3(REMAP_THREADS), 0, fs, g, n, mx, my, s.index.get());
  HIPCHK(c, hipGetLastError());
  s.r.geom = g, s.r.indexed = true;
  return LFVIO_OK;
}

// The gather of a source image of geometry g, already on the device, through the RESIDENT maps (valid: the caller's check) into dst
// [height][width * g.bpp], behind remap_index_for.  lfvio_remap_apply and lfvio_cloud_fuse (fuse.inc) enqueue it on the feature
// stream fs.
static int remap_gather(lfvio_ctx *c, hipStream_t fs, const RemapGeom &g, const unsigned char *src, unsigned char *dst) {
  lfvio_ctx::RemapState &s = c->remap;
  const size_t n = (size_t)s.r.width * s.r.height;
  if (int rc = remap_index_for(c, fs, g)) return rc;
  remap_apply_launch(fs, g.bpp, s.index.get(), src, dst, n);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int lfvio_remap_apply(lfvio_ctx *c, const LfvioImageFormat *fmt, int src_width, int src_height, const unsigned char *pixels, unsigned char *out) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = remap_apply_check(fmt, src_width, src_height, pixels, out)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  lfvio_ctx::RemapState &s = c->remap;
  if (!s.r.valid) {
    c->err = "lfvio_remap_apply: no resident map";
    return LFVIO_ERR_ARG;
  }
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  const LfvioImageFormat &f = fmt ? *fmt : mono;
  const RemapGeom g = remap_geom(f, src_width, src_height);
  const size_t n = (size_t)s.r.width * s.r.height, nI = imgfmt_bytes(f, src_width, src_height), nO = n * (size_t)g.bpp;
  FeatStage st(c);
  const size_t oI = st.take(nI), in_end = st.end, oO = st.take(nO);
  if (int rc = st.reserve()) return rc;
  std::memcpy(st.h + oI, pixels, nI);
  if (int rc = st.up(in_end)) return rc;
  if (int rc = remap_gather(c, st.fs, g, (const unsigned char *)(st.d + oI), (unsigned char *)(st.d + oO))) return rc;
  if (int rc = st.down(oO, st.end)) return rc;
  std::memcpy(out, st.h + oO, nO);
  return LFVIO_OK;
}

int lfvio_remap_reset(lfvio_ctx *c) {
  if (!c) return LFVIO_ERR_ARG;
  c->remap.r = RemapResident{};  // (the buffers stay: grow-only)
  return LFVIO_OK;
}
