// image_format.h — the encodings of lfvio_image_format_set / lfvio_image_gray (include/lfvio.h) and of the type-10 record
// (host/replay.h): bytes per pixel, the argument check, the grey value of a pixel and a whole image on the host.  Plain C++ (no HIP);
// the per-pixel functions are __host__ __device__ under hipcc, so k_img_gray (kernels_imgfmt.h) and the host run the same text.
// imgfmt.inc and host/replay.cpp use it, tests/test_image_format_ref.py compiles it alone with g++ and holds it to tests/image_ref.py,
// tests/tools/image_format_walk.cpp walks it under the CPU sanitizers.
//
//   code  name                              bytes / pixel  grey value
//   0     LFVIO_IMG_MONO8 (also 8UC1)       1              v
//   2     LFVIO_IMG_BGR8                    3              (1868 B + 9617 G + 4899 R + 8192) >> 14
//   3     LFVIO_IMG_RGB8                    3              the same on R, G, B in their places
//   4     LFVIO_IMG_BGRA8                   4              the same; the fourth byte is never read into the value
//   5     LFVIO_IMG_RGBA8                   4              the same
//   6     LFVIO_IMG_MONO16 (little endian)  2              (v + 128) / 257, integer division
//   7     LFVIO_IMG_MONO16_BE               2              the same after the byte swap
//
// The colour line is OpenCV 3.3's 8-bit RGB2Gray (14-bit coefficients 0.114, 0.587, 0.299, the rounding constant folded into its
// table), which cv_bridge::toCvCopy(msg, MONO8) calls; the 16-bit line is cv_bridge's convertTo(..., CV_8U, 255. / 65535.), whose
// rint(float32(v) * float32(255 / 65535)) equals (v + 128) / 257 for all 65 536 values.  BOTH ARE WRITTEN DOWN FROM MEMORY of those
// libraries: no OpenCV was at hand and nobody has compared them.  tests/image_ref.py is the specification.
#pragma once
#include <cstddef>

#include "../../include/lfvio.h"

#if defined(__HIPCC__)
#define IMGFMT_HD __host__ __device__ inline
#else
#define IMGFMT_HD inline
#endif

constexpr int IMGFMT_MIN_SIDE = 16, IMGFMT_MAX_SIDE = 8192;

// bytes per pixel of a code; 0: the code is not in the table
IMGFMT_HD int imgfmt_bpp(int code) {
  switch (code) {
    case LFVIO_IMG_MONO8: return 1;
    case LFVIO_IMG_BGR8:
    case LFVIO_IMG_RGB8: return 3;
    case LFVIO_IMG_BGRA8:
    case LFVIO_IMG_RGBA8: return 4;
    case LFVIO_IMG_MONO16:
    case LFVIO_IMG_MONO16_BE: return 2;
    default: return 0;
  }
}

// nullptr, or what is wrong with a setting whatever the image's size
inline const char *imgfmt_set_check(const LfvioImageFormat &f) {
  if (!imgfmt_bpp(f.encoding)) return "image format: an encoding outside the table (0, 2 .. 7)";
  if (f.step < 0 || f.step > LFVIO_IMG_MAX_STEP) return "image format: step negative or above 65536";
  return nullptr;
}
// ... and beside an image of width x height
inline const char *imgfmt_check(const LfvioImageFormat &f, int width, int height) {
  if (const char *why = imgfmt_set_check(f)) return why;
  if (width < IMGFMT_MIN_SIDE || width > IMGFMT_MAX_SIDE || height < IMGFMT_MIN_SIDE || height > IMGFMT_MAX_SIDE)
    return "image format: width or height outside [16, 8192]";
  if (f.step > 0 && f.step < width * imgfmt_bpp(f.encoding)) return "image format: step below width * bytes per pixel";
  return nullptr;
}
// bytes of one row of a checked format (step 0: the pixels alone), and of the image
inline size_t imgfmt_step(const LfvioImageFormat &f, int width) { return f.step > 0 ? (size_t)f.step : (size_t)width * (size_t)imgfmt_bpp(f.encoding); }
inline size_t imgfmt_bytes(const LfvioImageFormat &f, int width, int height) { return (size_t)height * imgfmt_step(f, width); }
// mono8 with contiguous rows: the bytes are the grey image, the same as no format
inline bool imgfmt_plain(const LfvioImageFormat &f, int width) { return f.encoding == LFVIO_IMG_MONO8 && (f.step == 0 || f.step == width); }

// What a call that takes a width x height image does under the setting f (nullptr: none; otherwise checked beside this size): the
// bytes that go up, and whether they are converted on the way into level 0
struct ImgfmtPlan {
  int code;
  size_t step, bytes;
  bool convert;  // false: the bytes are the grey image, exactly the call without a format
};
inline ImgfmtPlan imgfmt_plan(const LfvioImageFormat *f, int width, int height) {
  if (!f || imgfmt_plain(*f, width)) return ImgfmtPlan{LFVIO_IMG_MONO8, (size_t)width, (size_t)width * (size_t)height, false};
  return ImgfmtPlan{f->encoding, imgfmt_step(*f, width), imgfmt_bytes(*f, width, height), true};
}

// ---- the grey value of one pixel
IMGFMT_HD unsigned imgfmt_gray_bgr(unsigned b, unsigned g, unsigned r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }
IMGFMT_HD unsigned imgfmt_gray_16(unsigned v) { return (v + 128u) / 257u; }
// ... from the pixel's first three bytes b0, b1, b2 in memory order (a shorter pixel ignores the rest; a fourth byte is never asked for)
IMGFMT_HD unsigned imgfmt_gray(int code, unsigned b0, unsigned b1, unsigned b2) {
  switch (code) {
    case LFVIO_IMG_BGR8:
    case LFVIO_IMG_BGRA8: return imgfmt_gray_bgr(b0, b1, b2);
    case LFVIO_IMG_RGB8:
    case LFVIO_IMG_RGBA8: return imgfmt_gray_bgr(b2, b1, b0);
    case LFVIO_IMG_MONO16: return imgfmt_gray_16(b0 | (b1 << 8));
    case LFVIO_IMG_MONO16_BE: return imgfmt_gray_16(b1 | (b0 << 8));
    default: return b0;
  }
}

// ---- a whole image on the host: `height` rows of `step` bytes at src (a checked code, step >= width * bytes per pixel) into width x
// height grey bytes at dst.  Reads width * bytes per pixel bytes of every row and nothing else.
inline void imgfmt_to_gray(int code, int width, int height, size_t step, const unsigned char *src, unsigned char *dst) {
  const int bpp = imgfmt_bpp(code);
  for (int y = 0; y < height; y++) {
    const unsigned char *p = src + (size_t)y * step;
    unsigned char *o = dst + (size_t)y * (size_t)width;
    for (int x = 0; x < width; x++, p += bpp) o[x] = (unsigned char)imgfmt_gray(code, p[0], bpp > 1 ? p[1] : 0u, bpp > 2 ? p[2] : 0u);
  }
}
