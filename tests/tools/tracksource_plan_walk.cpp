// tracksource_plan_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/tracksource_plan.h and the lift of LFVIO_CAM_EQUIRECT
// (camera_models.h) for a sanitizer build of the host side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/tracksource_plan_walk.cpp -o tracksource_plan_walk        (one line)
//   ./tracksource_plan_walk
// An equirectangular map through a small OCam camera and a perspective map through a pinhole camera whose M sends part of the output
// outside the source, at 131 x 67 (8777 pixels: 1 mod 4, the last lane takes a tail of one) and 128 x 64, from a 161 x 123 source in
// every encoding with and without a padded odd step: the integer map by remap_offset, then EVERY lane of the launch through
// tracksource_lane — the host's copy of what k_remap_gray does — with the integer map, the source and level 0 in arrays of exactly
// imap: W * H ints, source: src_height * step bytes, level 0: W * H bytes, so a read or a write outside them is the sanitizer's to
// report; the result against imgfmt_to_gray of the host's nearest remap.  Then every refusal of tracksource_call_check beside an
// accepted neighbour, the plan's bytes, the launch geometry at the smallest and the largest size, and the EQUIRECT camera: its check,
// proj_check's refusal and the lift at the corners, the poles' rows and non-finite pixels.  Exit code 1 when something is not as expected.
#include <cstdio>
#include <limits>
#include <vector>

#include "tracksource_plan.h"

static int bad = 0;
static void wrong(const char *what) { std::printf("WRONG: %s\n", what), bad++; }
static const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf_ = std::numeric_limits<double>::infinity();

static LfvioCamera blank(int model) {  // everything NaN: a field the header must not read
  LfvioCamera k;
  k.model = model, k.cx = k.cy = k.c = k.d = k.e = k.fx = k.fy = k.k1 = k.k2 = k.p1 = k.p2 = k.xi = nan_;
  for (double &p : k.poly) p = nan_;
  return k;
}

int main() {
  const int SW = 161, SH = 123;
  const double s = 1280.0 / SW;
  // the PAL camera of an image s times smaller (pixel quantities divided by s)
  LfvioCamera pal = blank(LFVIO_CAM_OCAM);
  const double poly[5] = {-2.445239e+02, 0.0, 1.748610e-03, -1.757770e-06, 4.475965e-09};
  const double inv[14] = {376.845565, 246.746504, 19.035187, 23.840497, 18.991943, 6.066253, 1.560387, 5.854280, 3.458320, -1.995166, -1.509264,
                          1.089614, 1.340245, 0.255323};
  pal.cx = 645.107791 / s, pal.cy = 486.025172 / s, pal.c = 1.0, pal.d = 0.0, pal.e = 0.0;
  double sp = 1.0 / s;
  for (int i = 0; i < 5; i++) pal.poly[i] = poly[i] * sp, sp *= s;
  LfvioProjector pal_proj;
  pal_proj.camera = &pal;
  for (int i = 0; i < LFVIO_OCAM_INV_POLY_SIZE; i++) pal_proj.inv_poly[i] = i < 14 ? inv[i] / s : 0.0;
  LfvioCamera pin = blank(LFVIO_CAM_PINHOLE);
  pin.fx = 461.6 / (752.0 / SW), pin.fy = 460.3 / (752.0 / SW), pin.cx = 363.0 / (752.0 / SW), pin.cy = 248.1 / (752.0 / SW), pin.k1 = pin.k2 = pin.p1 = pin.p2 = 0.0;
  LfvioProjector pin_proj;
  pin_proj.camera = &pin;
  for (double &v : pin_proj.inv_poly) v = nan_;
  if (proj_check(&pal_proj) || proj_check(&pin_proj)) wrong("a projector of the walk is refused");
  // M = K^-1 behind a shift of the output pixel by (-20, 70)
  const double M[9] = {1.0 / pin.fx, 0.0, (-20.0 - pin.cx) / pin.fx, 0.0, 1.0 / pin.fy, (70.0 - pin.cy) / pin.fy, 0.0, 0.0, 1.0};

  const int encodings[] = {LFVIO_IMG_MONO8, LFVIO_IMG_BGR8, LFVIO_IMG_RGB8, LFVIO_IMG_BGRA8, LFVIO_IMG_RGBA8, LFVIO_IMG_MONO16, LFVIO_IMG_MONO16_BE};
  long pixels_done = 0, inside_all = 0, outside_all = 0, lanes_all = 0;
  for (int kind : {LFVIO_MAP_EQUIRECT, LFVIO_MAP_PERSPECTIVE})
    for (int size = 0; size < 2; size++) {
      const int W = size ? 128 : 131, H = size ? 64 : 67;
      const size_t n = (size_t)W * H;
      const ProjCam pc = proj_cam(kind == LFVIO_MAP_EQUIRECT ? pal_proj : pin_proj);
      std::vector<float> mx(n), my(n);
      for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
          const RemapEntry e = remap_entry(pc, kind, W, H, M, i, j);
          mx[(size_t)j * W + i] = e.x, my[(size_t)j * W + i] = e.y;
        }
      for (int enc : encodings)
        for (int pad : {0, 1}) {
          const int bpp = imgfmt_bpp(enc);
          const LfvioImageFormat fmt = {enc, pad ? SW * bpp + 5 + bpp % 2 : 0};
          TrackSourceState st;
          st.on = true, st.sw = SW, st.sh = SH;
          RemapResident r;
          r.valid = true, r.width = W, r.height = H;
          if (tracksource_call_check(st, r, &fmt, W, H)) wrong("a valid call is refused");
          const TrackSourcePlan plan = tracksource_plan(st, &fmt);
          if (plan.bytes != imgfmt_bytes(fmt, SW, SH) || plan.code != enc || !(plan.g == remap_geom(fmt, SW, SH))) wrong("tracksource_plan");
          std::vector<unsigned char> src(plan.bytes), level0(n), remapped(n * (size_t)bpp), want(n);
          for (size_t k = 0; k < src.size(); k++) src[k] = (unsigned char)(1 + (k * 7 + k / 251) % 255);
          std::vector<int> imap(n);
          long inside = 0;
          for (size_t p = 0; p < n; p++) {
            const int o = imap[p] = remap_offset(mx[p], my[p], plan.g);
            if (o >= 0 && (size_t)o + (size_t)bpp > src.size()) wrong("an offset behind the source image");
            for (int k = 0; k < bpp; k++) remapped[p * (size_t)bpp + k] = o < 0 ? 0 : src[(size_t)o + k];
            inside += o >= 0;
          }
          if (inside == 0 || inside == (long)n) wrong("a map without inside or without outside entries");
          imgfmt_to_gray(enc, W, H, (size_t)W * bpp, remapped.data(), want.data());
          const size_t lanes = tracksource_lanes(n);
          if (lanes * REMAP_RUN < n || lanes % REMAP_THREADS) wrong("tracksource_lanes");
          for (size_t lane = 0; lane < lanes; lane++) tracksource_lane(enc, imap.data(), src.data(), level0.data(), n, lane);
          if (level0 != want) wrong("level 0 is not the grey image of the remapped one");
          pixels_done += (long)n, inside_all += inside, outside_all += (long)n - inside, lanes_all += (long)lanes;
        }
    }

  // the per-call check
  {
    TrackSourceState off, on;
    on.on = true, on.sw = SW, on.sh = SH;
    RemapResident none, r;
    r.valid = true, r.width = 131, r.height = 67;
    const LfvioImageFormat bgr = {LFVIO_IMG_BGR8, 0}, bad_code = {1, 0}, short_step = {LFVIO_IMG_BGR8, 482}, exact = {LFVIO_IMG_BGR8, 483}, long_step = {LFVIO_IMG_BGR8, 65537};
    if (tracksource_call_check(off, none, &bad_code, 1, 1)) wrong("the setting off refuses");
    if (tracksource_call_check(on, r, &bgr, 131, 67) || tracksource_call_check(on, r, nullptr, 131, 67) || tracksource_call_check(on, r, &exact, 131, 67)) wrong("a valid call is refused");
    if (!tracksource_call_check(on, none, &bgr, 131, 67)) wrong("no resident map is accepted");
    if (!tracksource_call_check(on, r, &bgr, 130, 67) || !tracksource_call_check(on, r, &bgr, 131, 66) || !tracksource_call_check(on, r, &bgr, SW, SH)) wrong("a map of another size is accepted");
    if (!tracksource_call_check(on, r, &bad_code, 131, 67) || !tracksource_call_check(on, r, &short_step, 131, 67) || !tracksource_call_check(on, r, &long_step, 131, 67))
      wrong("a format is not judged beside the source");
    for (int side : {15, 8193, 0, -1}) {
      TrackSourceState t = on;
      t.sw = side;
      if (!tracksource_call_check(t, r, &bgr, 131, 67) || !remap_side_check(side, SH)) wrong("a source width outside [16, 8192] is accepted");
      t.sw = SW, t.sh = side;
      if (!tracksource_call_check(t, r, nullptr, 131, 67) || !remap_side_check(SW, side)) wrong("a source height outside [16, 8192] is accepted");
    }
    TrackSourceState big = on;
    big.sw = big.sh = 8192;
    const LfvioImageFormat bgra = {LFVIO_IMG_BGRA8, 0};
    if (tracksource_call_check(big, r, &bgra, 131, 67) || tracksource_plan(big, &bgra).bytes != (size_t)8192 * 8192 * 4) wrong("8192 x 8192 bgra8");
    for (size_t n : {(size_t)256, (size_t)257, (size_t)8192 * 8192}) {
      const size_t b = tracksource_blocks(n);
      if (b * REMAP_THREADS * REMAP_RUN < n || (b - 1) * REMAP_THREADS * REMAP_RUN >= n) wrong("the launch geometry");
    }
  }

  // LFVIO_CAM_EQUIRECT: the check, the projector's refusal, the lift
  long lifted = 0, nans = 0;
  {
    LfvioCamera eq = blank(LFVIO_CAM_EQUIRECT);
    eq.fx = 131.0, eq.fy = 67.0;
    if (track_camera_check(&eq)) wrong("a valid EQUIRECT camera is refused");
    LfvioProjector p;
    p.camera = &eq;
    for (double &v : p.inv_poly) v = nan_;
    if (!proj_check(&p)) wrong("proj_check accepts LFVIO_CAM_EQUIRECT");
    for (double v : {15.0, 8193.0, 100.5, nan_, inf_, -inf_, 0.0, -131.0}) {
      LfvioCamera k = eq;
      k.fx = v;
      if (!track_camera_check(&k)) wrong("an fx outside the integers of [16, 8192] is accepted");
      k.fx = 131.0, k.fy = v;
      if (!track_camera_check(&k)) wrong("an fy outside the integers of [16, 8192] is accepted");
    }
    for (double v : {16.0, 8192.0}) {
      LfvioCamera k = eq;
      k.fx = k.fy = v;
      if (track_camera_check(&k)) wrong("16 or 8192 is refused");
    }
    const TrackCam t = track_cam(eq);
    const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
    const float xs[] = {0.0f, 0.5f, 65.5f, 130.0f, 131.0f, -50.0f, 181.0f, -0.0f, 1e-40f, 3e38f, -3e38f, finf, -finf, fnan};
    const float ys[] = {0.0f, 33.5f, 66.0f, 67.0f, -50.0f, 117.0f, -0.0f, 1e-40f, 3e38f, finf, -finf, fnan};
    for (float x : xs)
      for (float y : ys) {
        double b[3];
        cam_bearing(t, x, y, b);
        const CamUndistorted u = cam_undistorted(t, x, y);
        const bool finite_in = std::isfinite(x) && std::isfinite(y) && std::fabs(x) < 1e6f && std::fabs(y) < 1e6f;
        const double n2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
        if (finite_in && !(std::fabs(n2 - 1.0) < 1e-12)) wrong("a bearing that is not a unit vector");
        lifted++, nans += (b[0] != b[0]) || (u.bx != u.bx);
      }
    for (int j = 0; j < 67; j++)
      for (int i = 0; i < 131; i++) {
        const CamRay a = cam_lift(t, (float)i, (float)j), m = remap_ray(LFVIO_MAP_EQUIRECT, 131, 67, nullptr, i, j);
        if (a.x != m.x || a.y != m.y || a.z != m.z) wrong("the lift at an integer pixel is not the map's ray");
      }
    if (nans == 0 || nans == lifted) wrong("the special pixels gave no NaN, or nothing else");
  }
  std::printf("tracksource_plan walk: %ld pixels through %ld lanes (%ld inside, %ld outside), %ld lifts (%ld NaN), %d wrong\n", pixels_done, lanes_all, inside_all,
              outside_all, lifted, nans, bad);
  return bad ? 1 : 0;
}
