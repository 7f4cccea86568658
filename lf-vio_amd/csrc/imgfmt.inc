// imgfmt.inc — host side of lfvio_image_format_set / lfvio_image_gray (include/lfvio.h) and of the conversion step of lfvio_klt_track
// (klt.inc): what cv_bridge::toCvCopy(img_msg, MONO8) does in front of FeatureTracker::readImage (feature_tracker_node.cpp:64-78) on
// the kernel of kernels_imgfmt.h.  Included by lfvio_hip.hip inside its extern "C" block, behind clahe.inc and in front of klt.inc.
//
// The setting only changes what `image` points to: imgfmt_plan (image_format.h) gives the bytes that go up and whether k_img_gray
// stands where the device-to-device copy into level 0 stood.  lfvio_track_batch_format is in trackbatch.inc.

// nullptr, or why a call on a W x H image is refused under the setting
static const char *imgfmt_call_check(const lfvio_ctx::ImageFormatState &s, int W, int H) { return s.on ? imgfmt_check(s.f, W, H) : nullptr; }

static int imgfmt_set(lfvio_ctx *c, lfvio_ctx::ImageFormatState &s, const LfvioImageFormat *fmt) {
  if (!fmt) {
    s.on = false;
    return LFVIO_OK;
  }
  if (const char *why = imgfmt_set_check(*fmt)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  s.f = *fmt, s.on = true;
  return LFVIO_OK;
}

// `src` (device: H rows of p.step bytes) into W x H grey bytes at dst, on fs
static int imgfmt_run(lfvio_ctx *c, hipStream_t fs, const ImgfmtPlan &p, int W, int H, const unsigned char *src, unsigned char *dst) {
  hipLaunchKernelGGL(k_img_gray, dim3((W + IMG_COLS - 1) / IMG_COLS, (H + IMG_ROWS - 1) / IMG_ROWS), dim3(IMG_THREADS), 0, fs, p.code, src, p.step, dst, W, H);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int lfvio_image_format_set(lfvio_ctx *c, const LfvioImageFormat *fmt) {
  if (!c) return LFVIO_ERR_ARG;
  return imgfmt_set(c, c->imgfmt, fmt);
}

int lfvio_image_gray(lfvio_ctx *c, const LfvioImageFormat *fmt, int width, int height, const unsigned char *pixels, unsigned char *out) {
  if (!c || !pixels || !out) return LFVIO_ERR_ARG;
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  const LfvioImageFormat &f = fmt ? *fmt : mono;
  if (const char *why = imgfmt_check(f, width, height)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  ImgfmtPlan p = imgfmt_plan(&f, width, height);
  p.convert = true;  // (mono8 with contiguous rows too: the kernel copies)
  const size_t nO = (size_t)width * height;
  FeatStage st(c);
  const size_t oI = st.take(p.bytes), in_end = st.end, oO = st.take(nO);
  if (int rc = st.reserve()) return rc;
  std::memcpy(st.h + oI, pixels, p.bytes);
  if (int rc = st.up(in_end)) return rc;
  if (int rc = imgfmt_run(c, st.fs, p, width, height, (const unsigned char *)(st.d + oI), (unsigned char *)(st.d + oO))) return rc;
  if (int rc = st.down(oO, st.end)) return rc;
  std::memcpy(out, st.h + oO, nO);
  return LFVIO_OK;
}
