// fuse.inc — host side of lfvio_cloud_fuse (include/lfvio.h, DESIGN.md 3x) on the kernels of kernels_fuse.h: a lidar scan's points into
// the camera frame, onto their pixels of the expanded image (or of the camera's own), the range image, the colours under the points
// and the painted image.  Included by lfvio_hip.hip inside its extern "C" block, behind remap.inc.
//
// Every check is fuse_plan.h's, or the resident map's, and runs before anything is touched.  Cloud, image and every output travel
// through the staging block of feat.inc (the context's grow-only buffers): ONE copy up — [cloud | image] —, the launches back to back
// on the feature stream, ONE copy down — the outputs asked for, laid out next to each other; what a later launch needs and nobody asked
// for (the remapped image under `colour`, say) lies behind them and stays on the device.  A GIVEN image is packed row by row on its way
// into the staging block, so the device sees contiguous rows and, where image_out is asked for, the copy down starts at that image.
// The REMAP path is lfvio_remap_apply's own (remap_gather of remap.inc).  No tracker state is touched.

int lfvio_cloud_fuse(lfvio_ctx *c, const LfvioFuseIn *in, LfvioFuseOut *out) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = fuse_check(in, out)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  lfvio_ctx::RemapState &s = c->remap;
  const bool given = in->image_mode == LFVIO_FUSE_IMAGE_GIVEN, remap = in->image_mode == LFVIO_FUSE_IMAGE_REMAP;
  if (remap && !s.r.valid) {
    c->err = "lfvio_cloud_fuse: no resident map";
    return LFVIO_ERR_ARG;
  }
  if (remap && (s.r.width != in->width || s.r.height != in->height)) {
    c->err = "lfvio_cloud_fuse: the resident map is of another size";
    return LFVIO_ERR_ARG;
  }
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  const LfvioImageFormat &f = in->fmt ? *in->fmt : mono;
  const int n = in->n, bpp = (given || remap) ? imgfmt_bpp(f.encoding) : 0;
  const size_t pixels = (size_t)in->width * in->height;
  const size_t nC = (size_t)n * in->point_step, row = (size_t)in->width * bpp, nImg = pixels * bpp;
  const size_t nSrc = remap ? imgfmt_bytes(f, in->src_width, in->src_height) : 0;
  const size_t nIdx = (size_t)n * sizeof(int), nRange = pixels * sizeof(float), nCol = (size_t)n * bpp, nCnt = 3 * sizeof(int);
  const bool paint = bpp && in->paint_on && out->image_out;  // (an image nobody receives is not painted)

  // the staging block: [cloud | src (REMAP) or image (GIVEN)] up; [image?] counts [index?] [range?] [colour?] down; the rest device only
  FeatStage st(c);
  const size_t oC = st.take(nC);
  const size_t oSrc = remap ? st.take(nSrc) : 0;
  size_t oImg = given ? st.take(nImg) : 0;
  const size_t in_end = st.end;
  if (remap && out->image_out) oImg = st.take(nImg);
  const size_t oCnt = st.take(nCnt);
  const size_t from = ((given || remap) && out->image_out) ? oImg : oCnt;
  const size_t oIdx = out->index ? st.take(nIdx) : 0, oRange = out->range ? st.take(nRange) : 0, oCol = out->colour ? st.take(nCol) : 0;
  const size_t to = st.end;
  const size_t oIdxDev = out->index ? oIdx : st.take(nIdx);
  if (remap && !out->image_out && out->colour) oImg = st.take(nImg);
  if (int rc = st.reserve()) return rc;

  if (nC) std::memcpy(st.h + oC, in->cloud, nC);
  if (remap) std::memcpy(st.h + oSrc, in->pixels, nSrc);
  if (given) {
    const size_t step = imgfmt_step(f, in->width);
    for (int j = 0; j < in->height; j++) std::memcpy(st.h + oImg + (size_t)j * row, in->pixels + (size_t)j * step, row);
  }
  if (in_end)
    if (int rc = st.up(in_end)) return rc;

  unsigned char *img = (unsigned char *)(st.d + oImg);
  if (remap && (out->image_out || out->colour))
    if (int rc = remap_gather(c, st.fs, remap_geom(f, in->src_width, in->src_height), (const unsigned char *)(st.d + oSrc), img)) return rc;
  HIPCHK(c, hipMemsetAsync(st.d + oCnt, 0, nCnt, st.fs));
  unsigned *range = out->range ? (unsigned *)(st.d + oRange) : nullptr;
  if (range) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)range, (int)FUSE_INF_BITS, pixels, st.fs));
  if (n > 0) {
    const dim3 grid(fuse_blocks(n)), block(FUSE_THREADS);
    int *index = (int *)(st.d + oIdxDev);
    hipLaunchKernelGGL(k_fuse_project, grid, block, 0, st.fs, fuse_view(*in, &s.kb), fuse_layout(*in), n, (const unsigned char *)(st.d + oC), index, range,
                       (int *)(st.d + oCnt));
    HIPCHK(c, hipGetLastError());
    if (out->colour) {
      hipLaunchKernelGGL(k_fuse_sample, grid, block, 0, st.fs, n, bpp, (const int *)index, (const unsigned char *)img, (unsigned char *)(st.d + oCol));
      HIPCHK(c, hipGetLastError());
    }
    if (paint) {
      const unsigned p4 = (unsigned)in->paint[0] | ((unsigned)in->paint[1] << 8) | ((unsigned)in->paint[2] << 16) | ((unsigned)in->paint[3] << 24);
      hipLaunchKernelGGL(k_fuse_paint, grid, block, 0, st.fs, n, bpp, p4, (const int *)index, img);
      HIPCHK(c, hipGetLastError());
    }
  }
  if (int rc = st.down(from, to)) return rc;
  if (out->image_out) std::memcpy(out->image_out, st.h + oImg, nImg);
  if (out->counts) std::memcpy(out->counts, st.h + oCnt, nCnt);
  if (out->index && nIdx) std::memcpy(out->index, st.h + oIdx, nIdx);
  if (out->range) std::memcpy(out->range, st.h + oRange, nRange);
  if (out->colour && nCol) std::memcpy(out->colour, st.h + oCol, nCol);
  return LFVIO_OK;
}
