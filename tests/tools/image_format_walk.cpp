// image_format_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/image_format.h for a CPU sanitizer build of the host side of
// lfvio_image_format_set / lfvio_image_gray and of the type-10 loader: for every code, in and outside the table, at odd sizes and
// steps it runs imgfmt_check and, where the format is accepted, imgfmt_plan and the whole-image converter on a source block of
// EXACTLY the planned bytes and a destination of exactly width * height — a read past a row's pixels in the last row, or a write
// past the image, lands outside the allocation, where AddressSanitizer sees it.  The grey bytes are compared with the table's formulas
// written out again here.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc tests/tools/image_format_walk.cpp -o walk && ./walk
//
// Prints the number of images walked and exits 0; anything else is a finding.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "image_format.h"

static int fail(const char *what, int code, int w, int h, int step) {
  std::fprintf(stderr, "image_format_walk: %s (code %d, %d x %d, step %d)\n", what, code, w, h, step);
  return 1;
}

static unsigned char by_hand(int code, const unsigned char *p) {
  auto bgr = [](unsigned b, unsigned g, unsigned r) { return (unsigned char)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14); };
  switch (code) {
    case 0: return p[0];
    case 2:
    case 4: return bgr(p[0], p[1], p[2]);
    case 3:
    case 5: return bgr(p[2], p[1], p[0]);
    case 6: return (unsigned char)(((unsigned)p[0] + 256u * p[1] + 128u) / 257u);
    default: return (unsigned char)(((unsigned)p[1] + 256u * p[0] + 128u) / 257u);
  }
}

int main() {
  const int sizes[][2] = {{16, 16}, {17, 19}, {31, 16}, {64, 48}, {80, 60}, {161, 123}};
  const int bpp_of[8] = {1, 0, 3, 3, 4, 4, 2, 2};
  long walked = 0, refused = 0;
  unsigned seed = 2463534242u;
  auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
  for (int code = -2; code <= 10; code++) {
    const int bpp = code >= 0 && code < 8 ? bpp_of[code] : 0;
    if (imgfmt_bpp(code) != bpp) return fail("bytes per pixel", code, 0, 0, 0);
    for (const auto &wh : sizes) {
      const int w = wh[0], h = wh[1], row = w * (bpp ? bpp : 1);
      const int steps[] = {-1, 0, 1, row - 1, row, row + 1, row + 3, row + 5, 512, LFVIO_IMG_MAX_STEP, LFVIO_IMG_MAX_STEP + 1};
      for (int step : steps) {
        const LfvioImageFormat f = {code, step};
        const bool ok = bpp && step >= 0 && step <= LFVIO_IMG_MAX_STEP && (step == 0 || step >= row);
        if ((imgfmt_check(f, w, h) == nullptr) != ok) return fail("imgfmt_check", code, w, h, step);
        if ((imgfmt_set_check(f) == nullptr) != (bpp && step >= 0 && step <= LFVIO_IMG_MAX_STEP)) return fail("imgfmt_set_check", code, w, h, step);
        if (!ok) {
          refused++;
          continue;
        }
        if (imgfmt_check(f, 15, h) == nullptr || imgfmt_check(f, w, 8193) == nullptr) return fail("a size outside [16, 8192] accepted", code, w, h, step);
        const ImgfmtPlan p = imgfmt_plan(&f, w, h);
        const size_t want_step = step ? (size_t)step : (size_t)row;
        if (p.step != want_step || p.bytes != want_step * (size_t)h || p.convert != !(code == 0 && want_step == (size_t)w) || (p.convert && p.code != code))
          return fail("imgfmt_plan", code, w, h, step);
        std::vector<unsigned char> src(p.bytes), dst((size_t)w * h, 0x5A);
        for (auto &b : src) b = (unsigned char)(next() >> 24);
        imgfmt_to_gray(code, w, h, p.step, src.data(), dst.data());
        for (int y = 0; y < h; y++)
          for (int x = 0; x < w; x++)
            if (dst[(size_t)y * w + x] != by_hand(code, src.data() + (size_t)y * p.step + (size_t)x * bpp)) return fail("a grey byte", code, w, h, step);
        walked++;
      }
    }
  }
  const ImgfmtPlan none = imgfmt_plan(nullptr, 80, 60);
  if (none.convert || none.bytes != 4800 || none.step != 80) return fail("imgfmt_plan without a format", 0, 80, 60, 0);
  std::printf("image_format_walk: %ld images converted, %ld formats refused\n", walked, refused);
  return 0;
}
