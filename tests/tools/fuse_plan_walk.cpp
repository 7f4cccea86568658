// fuse_plan_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/fuse_plan.h (the host side of lfvio_cloud_fuse) for a sanitizer build
// (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/fuse_plan_walk.cpp -o fuse_plan_walk        (one line)
//   ./fuse_plan_walk
// Clouds in heap arrays of exactly n * point_step bytes — so a read past a point's bytes is the sanitizer's to find — in the layouts of
// tests/test_fuse_plan.py (point_step 12, 13, 16, 22, 48, offsets permuted, both byte orders, by dwords where the layout allows it and byte
// by byte always): every field comes back as it was packed.  fuse_point over a lattice on the whole sphere and over special points
// (zeros, +-inf, NaN, the largest and a denormal float in each coordinate, the seam, the axes, the poles, |Z / nxy| >= 2^66), through
// three poses, EQUIRECT at 16 x 16, 33 x 17 and 8192 x 4096 and CAMERA through one camera of each model: a kept point's index is inside
// the image, a dropped one's is -1, and the host's copy of what the three kernels do — the minimum per pixel, the colour under a point,
// the paint — stays inside arrays of exactly the image's size.  Then every refusal of fuse_check and the launch geometry.  What the
// walk asserts is coarse: the bits are tests/test_fuse_plan.py's business.  Exit code 1 when something is not as expected.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "fuse_plan.h"

static int bad = 0;
static void wrong(const char *what, int a = 0, int b = 0) { std::printf("WRONG: %s (%d, %d)\n", what, a, b), bad++; }

static const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf_ = std::numeric_limits<double>::infinity();
static const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();

static LfvioCamera blank(int model, double cx, double cy) {  // everything else NaN: a field the header must not read
  LfvioCamera k;
  k.model = model, k.cx = cx, k.cy = cy, k.c = k.d = k.e = k.fx = k.fy = k.k1 = k.k2 = k.p1 = k.p2 = k.xi = nan_;
  for (double &p : k.poly) p = nan_;
  return k;
}
static LfvioCamera ocam() {
  LfvioCamera k = blank(LFVIO_CAM_OCAM, 32.0, 24.0);
  const double poly[5] = {-12.226195, 0.0, 3.49722e-02, -7.03108e-04, 3.580772e-05};  // the PAL polynomial of an image 20 times smaller
  k.c = 1.0, k.d = 0.0, k.e = 0.0;
  for (int i = 0; i < 5; i++) k.poly[i] = poly[i];
  return k;
}
static LfvioCamera plane(int model, double xi) {
  LfvioCamera k = blank(model, 31.5, 23.5);
  k.fx = 40.0, k.fy = 39.0, k.k1 = -0.28, k.k2 = 0.07, k.p1 = 2e-4, k.p2 = 2e-5;
  if (model == LFVIO_CAM_MEI) k.xi = xi;
  return k;
}
static LfvioCamera kb() {
  LfvioCamera k = blank(LFVIO_CAM_KANNALA_BRANDT, 31.0, 24.5);
  k.fx = 16.0, k.fy = 16.0, k.poly[0] = 0.0034823894022493434, k.poly[1] = 0.0007150348452162257, k.poly[2] = -0.0020532361418706202,
  k.poly[3] = 0.00020293673591811182;
  return k;
}
static LfvioProjector projector(const LfvioCamera *cam) {
  const double inv[14] = {376.845565, 246.746504, 19.035187, 23.840497, 18.991943, 6.066253, 1.560387, 5.854280, 3.458320, -1.995166, -1.509264,
                          1.089614, 1.340245, 0.255323};
  LfvioProjector p;
  p.camera = cam;
  for (int i = 0; i < LFVIO_OCAM_INV_POLY_SIZE; i++) p.inv_poly[i] = cam->model == LFVIO_CAM_OCAM ? (i < 14 ? inv[i] / 20.0 : 0.0) : nan_;
  return p;
}

static LfvioFuseIn base_in() {
  LfvioFuseIn in;
  std::memset(&in, 0, sizeof in);
  in.n = 1, in.point_step = 16, in.off_x = 0, in.off_y = 4, in.off_z = 8;
  in.R[0] = in.R[4] = in.R[8] = 1.0;
  in.max_range = inf_, in.kind = LFVIO_FUSE_EQUIRECT, in.width = 33, in.height = 17;
  return in;
}

static std::vector<float> cloud_points() {
  std::vector<float> P;
  auto add = [&](float x, float y, float z) { P.push_back(x), P.push_back(y), P.push_back(z); };
  for (int a = 0; a <= 24; a++)      // polar angle 0 .. pi: both poles are in
    for (int b = 0; b < 48; b++) {   // azimuth: the seam and the axes are in
      const double th = 3.14159265358979323846 * a / 24.0, ph = 6.283185307179586 * b / 48.0, r = 0.3 + 2.5 * ((a * 48 + b) % 47);
      add((float)(r * std::sin(th) * std::sin(ph)), (float)(r * std::sin(th) * std::cos(ph)), (float)(r * std::cos(th)));
    }
  const float sp[][3] = {{0, 0, 0}, {-0.0f, 0, -0.0f}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1e-30f, -1, 0}, {-1e-30f, -1, 0},
                         {0, 1e-25f, -1}, {0, 1e-25f, 1}, {1e-25f, 0, -1}, {1e-40f, 1e-40f, 1e-40f}, {3.4e38f, -3.4e38f, 3.4e38f}, {0.1f, -0.05f, 2}, {-0.1f, 0.05f, -2}};
  for (auto &p : sp) add(p[0], p[1], p[2]);
  const float odd[] = {fnan, finf, -finf, 3.4028235e38f, 1e-45f};
  for (int k = 0; k < 3; k++)
    for (float v : odd) {
      float p[3] = {1.0f, 2.0f, 0.5f};
      p[k] = v;
      add(p[0], p[1], p[2]);
    }
  return P;
}

// n points into exactly n * step heap bytes, 0xee in every byte that is no field
static unsigned char *pack(const std::vector<float> &P, int step, const int off[3], int big) {
  const size_t n = P.size() / 3;
  unsigned char *d = new unsigned char[n * (size_t)step];
  std::memset(d, 0xee, n * (size_t)step);
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) {
      unsigned char b[4];
      std::memcpy(b, &P[3 * i + k], 4);
      for (int j = 0; j < 4; j++) d[i * (size_t)step + off[k] + j] = big ? b[3 - j] : b[j];
    }
  return d;
}

static void walk_layouts(const std::vector<float> &P) {
  const int layouts[][4] = {{12, 0, 4, 8}, {12, 8, 0, 4}, {13, 9, 0, 4}, {16, 4, 8, 12}, {16, 12, 0, 8}, {22, 2, 6, 10}, {22, 18, 1, 9}, {48, 0, 4, 8}, {48, 44, 16, 0},
                            {48, 5, 21, 33}, {1024, 1020, 0, 512}};
  const size_t n = P.size() / 3;
  for (auto &l : layouts)
    for (int big = 0; big < 2; big++) {
      LfvioFuseIn in = base_in();
      in.point_step = l[0], in.off_x = l[1], in.off_y = l[2], in.off_z = l[3], in.big_endian = big, in.n = (int)n;
      unsigned char *d = pack(P, l[0], l + 1, big);
      in.cloud = d;
      const LfvioFuseOut out = {};
      if (fuse_check(&in, &out)) wrong("a layout is refused", l[0], l[1]);
      FuseLayout lay = fuse_layout(in);
      if (lay.dwords != ((l[0] | l[1] | l[2] | l[3]) % 4 == 0)) wrong("dwords", l[0], l[1]);
      for (int force = 0; force < 2; force++) {
        if (force) lay.dwords = 0;
        for (size_t i = 0; i < n; i++) {
          const FuseXYZ p = fuse_read(lay, d, i);
          if (std::memcmp(&p.x, &P[3 * i], 4) || std::memcmp(&p.y, &P[3 * i + 1], 4) || std::memcmp(&p.z, &P[3 * i + 2], 4)) wrong("a field", l[0], (int)i);
        }
      }
      delete[] d;
    }
}

// the host's copy of the three kernels on arrays of exactly the image's size
static void walk_view(const char *name, LfvioFuseIn in, const std::vector<float> &P, bool expect_kept) {
  const LfvioFuseOut none = {};
  in.n = (int)(P.size() / 3), in.cloud = (const unsigned char *)P.data();  // (read through fuse_point's arguments here, not as bytes)
  if (const char *why = fuse_check(&in, &none)) {
    std::printf("%s: %s\n", name, why);
    return wrong("a view is refused");
  }
  const FuseView v = fuse_view(in);
  const size_t n = P.size() / 3, pixels = (size_t)in.width * in.height;
  const int bpp = 3;
  std::vector<unsigned> range(pixels, FUSE_INF_BITS);
  std::vector<unsigned char> image(pixels * bpp, 7), colour(n * bpp, 0xee);
  std::vector<int> index(n);
  int counts[3] = {0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const FuseHit h = fuse_point(v, P[3 * i], P[3 * i + 1], P[3 * i + 2]);
    index[i] = h.index;
    if (h.why < 0 || h.why > 2) return wrong("why");
    counts[h.why]++;
    if ((h.why == FUSE_KEPT) != (h.index >= 0)) wrong(name, (int)i, h.index);
    if (h.index < -1 || h.index >= (int)pixels) wrong("index outside", (int)i, h.index);
    if (h.index >= 0) {
      unsigned bits;
      std::memcpy(&bits, &h.range, 4);
      if (!(h.range > 0.0f) || bits > FUSE_INF_BITS) wrong("a kept point's range", (int)i);
      if (bits < range.at((size_t)h.index)) range.at((size_t)h.index) = bits;
    }
  }
  for (size_t i = 0; i < n; i++)
    for (int b = 0; b < bpp; b++) colour.at(i * bpp + b) = index[i] < 0 ? 0 : image.at((size_t)index[i] * bpp + b);
  for (size_t i = 0; i < n; i++)
    if (index[i] >= 0)
      for (int b = 0; b < bpp; b++) image.at((size_t)index[i] * bpp + b) = 255;
  if (counts[0] + counts[1] + counts[2] != (int)n) wrong("counts");
  if (expect_kept && counts[FUSE_KEPT] * 4 < (int)n) wrong("few points kept", counts[FUSE_KEPT], (int)n);
  std::printf("%-28s %4d x %4d: kept %4d, gate %3d, projection %4d\n", name, in.width, in.height, counts[0], counts[1], counts[2]);
}

static void walk_points(const std::vector<float> &P) {
  const double th = 1.5707963267948966;
  const double poses[3][12] = {{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0},
                               {std::cos(th), -std::sin(th), 0, std::sin(th), -std::cos(th), 0, 0, 0, 1, 0, 0, -0.12},
                               {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6, 0.3, -0.2, 0.1}};
  const int sizes[3][2] = {{16, 16}, {33, 17}, {8192, 4096}};
  for (auto &pose : poses)
    for (auto &s : sizes)
      for (int gate = 0; gate < 2; gate++) {
        LfvioFuseIn in = base_in();
        for (int k = 0; k < 9; k++) in.R[k] = pose[k];
        for (int k = 0; k < 3; k++) in.T[k] = pose[9 + k];
        in.width = s[0], in.height = s[1];
        if (gate) in.min_range = 5.0, in.max_range = 60.0;
        walk_view(gate ? "equirect, gate [5, 60]" : "equirect", in, P, !gate);
      }
  const LfvioCamera cams[5] = {ocam(), plane(LFVIO_CAM_PINHOLE, 0.0), plane(LFVIO_CAM_MEI, 2.057), plane(LFVIO_CAM_MEI, 0.5), kb()};
  const char *names[5] = {"camera OCAM", "camera PINHOLE", "camera MEI xi 2.057", "camera MEI xi 0.5", "camera KANNALA_BRANDT"};
  for (int c = 0; c < 5; c++) {
    const LfvioProjector p = projector(&cams[c]);
    LfvioFuseIn in = base_in();
    in.kind = LFVIO_FUSE_CAMERA, in.proj = &p, in.width = 64, in.height = 48;
    walk_view(names[c], in, P, false);
    // the point in front is kept, its mirror image through the centre is not (PINHOLE, MEI with xi < 1)
    const FuseView v = fuse_view(in);
    const FuseHit front = fuse_point(v, 0.1f, -0.05f, 2.0f), back = fuse_point(v, -0.1f, 0.05f, -2.0f);
    if (c == 1 || c == 3)
      if (front.why != FUSE_KEPT || back.why != FUSE_PROJECTION) wrong(names[c], front.why, back.why);
  }
}

static void walk_refusals() {
  const LfvioCamera cam = plane(LFVIO_CAM_PINHOLE, 0.0), zero_fx = [] { LfvioCamera k = plane(LFVIO_CAM_PINHOLE, 0.0); k.fx = 0.0; return k; }();
  const LfvioProjector proj = projector(&cam), bad_proj = projector(&zero_fx), no_cam = {nullptr, {}};
  unsigned char byte = 0;
  const LfvioImageFormat bgr = {LFVIO_IMG_BGR8, 0}, enc1 = {1, 0}, short_step = {LFVIO_IMG_BGR8, 98}, long_step = {LFVIO_IMG_BGR8, 65537};
  LfvioFuseOut none = {}, colour = {}, image = {};
  colour.colour = &byte, image.image_out = &byte;
  int checked = 0;
  auto expect = [&](bool refused, LfvioFuseIn in, const LfvioFuseOut *out, const char *what) {
    if (in.n > 0 && !in.cloud && std::strcmp(what, "null cloud")) in.cloud = &byte;
    if ((fuse_check(&in, out) != nullptr) != refused) wrong(what);
    checked++;
  };
  LfvioFuseIn in = base_in();
  expect(false, in, &none, "the base case");
  if (!fuse_check(nullptr, &none) || !fuse_check(&in, nullptr)) wrong("null in / out");
  expect(true, in, &none, "null cloud");
  in.n = 0, expect(false, in, &none, "n == 0 needs no cloud"), in = base_in();
  in.n = -1, expect(true, in, &none, "n < 0"), in.n = (1 << 20) + 1, expect(true, in, &none, "n > 1 << 20"), in.n = 1 << 20, expect(false, in, &none, "n == 1 << 20");
  in = base_in(), in.point_step = 11, expect(true, in, &none, "step 11"), in.point_step = 1025, in.off_z = 1021, expect(true, in, &none, "step 1025");
  in = base_in(), in.off_x = 13, expect(true, in, &none, "offset past the point"), in.off_x = -1, expect(true, in, &none, "negative offset");
  in = base_in(), in.off_y = 3, expect(true, in, &none, "fields overlap"), in.off_y = 12, expect(false, in, &none, "fields touch");
  in = base_in(), in.big_endian = 2, expect(true, in, &none, "big_endian 2");
  in = base_in(), in.R[5] = nan_, expect(true, in, &none, "NaN in R"), in = base_in(), in.T[2] = inf_, expect(true, in, &none, "inf in T");
  in = base_in(), in.min_range = -1.0, expect(true, in, &none, "min_range < 0"), in.min_range = nan_, expect(true, in, &none, "min_range NaN");
  in = base_in(), in.min_range = 2.0, in.max_range = 1.0, expect(true, in, &none, "max < min"), in.max_range = nan_, expect(true, in, &none, "max NaN");
  in.max_range = 2.0, expect(false, in, &none, "max == min");
  in = base_in(), in.kind = 2, expect(true, in, &none, "kind 2");
  in = base_in(), in.width = 15, expect(true, in, &none, "width 15"), in.width = 16, in.height = 8193, expect(true, in, &none, "height 8193");
  in = base_in(), in.kind = LFVIO_FUSE_CAMERA, expect(true, in, &none, "CAMERA without a projector");
  in.proj = &no_cam, expect(true, in, &none, "a projector without a camera"), in.proj = &bad_proj, expect(true, in, &none, "fx == 0");
  in.proj = &proj, expect(false, in, &none, "CAMERA");
  in = base_in(), in.image_mode = 3, expect(true, in, &none, "image_mode 3");
  in = base_in(), expect(true, in, &colour, "colour without an image"), expect(true, in, &image, "image_out without an image");
  for (int mode = LFVIO_FUSE_IMAGE_GIVEN; mode <= LFVIO_FUSE_IMAGE_REMAP; mode++) {
    in = base_in(), in.image_mode = mode, in.src_width = 33, in.src_height = 17;
    expect(true, in, &image, "null pixels");
    in.pixels = &byte, expect(false, in, &image, "a null format is mono8"), in.fmt = &bgr, expect(false, in, &colour, "bgr8");
    in.fmt = &enc1, expect(true, in, &image, "encoding 1"), in.fmt = &short_step, expect(true, in, &image, "step below a row");
    in.fmt = &long_step, expect(true, in, &image, "step above 65536");
  }
  in = base_in(), in.image_mode = LFVIO_FUSE_IMAGE_REMAP, in.pixels = &byte, in.src_width = 15, in.src_height = 48, expect(true, in, &image, "src_width 15");
  in.image_mode = LFVIO_FUSE_IMAGE_GIVEN, expect(false, in, &image, "GIVEN does not read src_width");
  if (fuse_blocks(0) != 0 || fuse_blocks(1) != 1 || fuse_blocks(256) != 1 || fuse_blocks(257) != 2 || fuse_blocks(1 << 20) != 4096) wrong("fuse_blocks");
  std::printf("%d verdicts of fuse_check\n", checked);
}

int main() {
  const std::vector<float> P = cloud_points();
  walk_layouts(P);
  walk_points(P);
  walk_refusals();
  std::printf(bad ? "%d things wrong\n" : "fuse_plan walk: clean (%d wrong)\n", bad);
  return bad ? 1 : 0;
}
