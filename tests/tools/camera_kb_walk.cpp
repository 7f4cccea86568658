// camera_kb_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/camera_kb.h and the KANNALA_BRANDT argument checks of track_plan.h for a
// sanitizer build of the host side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/camera_kb_walk.cpp -o camera_kb_walk        (one line)
//   ./camera_kb_walk
// The reference's three calibrations and the branch cameras of tests/kb_ref.py, each over a pixel grid that covers the image, 50 px
// beyond it, the principal point and NaN, +-inf, +-3e38 in either coordinate; every refused field, each alone; the constants' cache
// across a change of camera.  What the walk asserts is coarse (finite pixels inside the monotone range give a unit ray to 1e-12, the
// fallback is reached where it must be, the verdicts are the expected ones): the bits are tests/test_kb_ref.py's business.  The
// sanitizers see every conversion, shift and index on the way, the float-to-integer conversions the header promises not to make
// among them.  Exit code 1 when a verdict or a ray is not the expected one.
#include <cstdio>
#include <limits>
#include <vector>

#include "track_plan.h"

static int bad = 0;
static void wrong(const char *what) { std::printf("WRONG: %s\n", what), bad++; }

struct Calib {
  const char *name;
  int width, height;
  double k[4], mu, mv, u0, v0;
};

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Calib calibs[] = {
      {"TUM", 512, 512, {0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182}, 190.97847715128717,
       190.9733070521226, 254.93170605935475, 256.8974428996504},
      {"CLA", 752, 480, {-0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.02008469575876223}, 472.2863830700696,
       470.83759684346785, 368.8316828103749, 232.23688706965652},
      {"RSFISH", 640, 480, {1.7280355035195181e-02, -2.5505200860040985e-02, 2.2621441637715487e-02, -7.3355871719731113e-03},
       2.7723712054408202e+02, 2.7699784668734617e+02, 3.3625356873985868e+02, 2.3603924727453901e+02},
      {"KB_K5_0", 752, 480, {-0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.0}, 472.2863830700696, 470.83759684346785,
       368.8316828103749, 232.23688706965652},
      {"KB_K45_0", 752, 480, {-0.005740195474458931, 0.02878252863739417, 0.0, 0.0}, 472.2863830700696, 470.83759684346785, 368.8316828103749,
       232.23688706965652},
      {"KB_IDEAL", 752, 480, {0.0, 0.0, 0.0, 0.0}, 472.2863830700696, 470.83759684346785, 368.8316828103749, 232.23688706965652},
  };
  KbCache cache;
  long rays = 0, fallbacks = 0, nans = 0;
  for (const Calib &q : calibs) {
    LfvioCamera cam;  // every field the model does not read stays NaN
    cam.model = LFVIO_CAM_KANNALA_BRANDT, cam.cx = q.u0, cam.cy = q.v0, cam.c = cam.d = cam.e = nan;
    for (int i = 0; i < 4; i++) cam.poly[i] = q.k[i];
    cam.poly[4] = cam.k1 = cam.k2 = cam.p1 = cam.p2 = cam.xi = nan, cam.fx = q.mu, cam.fy = q.mv;
    if (track_common_check(&cam, 40)) wrong("a shipped calibration is refused");
    const TrackCam t = track_cam(cam, &cache), fresh = track_cam(cam), again = track_cam(cam, &cache);
    if (t.theta_lim != fresh.theta_lim || t.r_lim != fresh.r_lim || again.theta_lim != t.theta_lim || again.r_lim != t.r_lim) wrong("the cache");
    if (!(t.theta_lim > 0.0 && t.theta_lim <= 3.14159265358979323846) || !(t.r_lim > 0.0)) wrong("theta_lim or r_lim");
    std::printf("%-9s theta_lim %.17g r_lim %.17g\n", q.name, t.theta_lim, t.r_lim);
    std::vector<float> xs, ys;
    for (int x = -50; x <= q.width + 50; x += 7) xs.push_back((float)x + 0.25f);
    for (int y = -50; y <= q.height + 50; y += 7) ys.push_back((float)y + 0.5f);
    const float odd[] = {(float)nan, (float)inf, (float)-inf, 3e38f, -3e38f};
    xs.push_back((float)q.u0), ys.push_back((float)q.v0);
    for (float v : odd) xs.push_back(v), ys.push_back(v);
    long cam_fallbacks = 0;
    for (float px : xs)
      for (float py : ys) {
        double X, Y, Z;
        kb_lift_pixel(t.inv11, t.inv13, t.inv22, t.inv23, t.poly, t.theta_lim, t.r_lim, px, py, X, Y, Z);
        rays++;
        const double x = t.inv11 * (double)px + t.inv13, y = t.inv22 * (double)py + t.inv23, r = std::sqrt(x * x + y * y);
        if (!(r <= t.r_lim)) cam_fallbacks++;
        if (X != X || Y != Y || Z != Z) {
          nans++;
          if (std::isfinite(px) && std::isfinite(py) && std::fabs(px) < 1e30f && std::fabs(py) < 1e30f) wrong("a NaN ray from an ordinary pixel");
          continue;
        }
        if (r <= t.r_lim && std::fabs(std::sqrt(X * X + Y * Y + Z * Z) - 1.0) > 1e-12) wrong("a ray that is not a unit vector");
        if (r <= t.r_lim && std::fabs(kb_f(t.poly, kb_root(t.poly, t.theta_lim, t.r_lim, r)) - r) > 1e-13 * (r > 1.0 ? r : 1.0)) wrong("a root that is none");
      }
    fallbacks += cam_fallbacks;
    if (q.name[0] == 'R' && cam_fallbacks < 100) wrong("RSFISH never reached the fallback");
    // every refused field, each alone; what the model does not read may be anything
    double *fields[8] = {&cam.cx, &cam.cy, &cam.fx, &cam.fy, &cam.poly[0], &cam.poly[1], &cam.poly[2], &cam.poly[3]};
    for (double *f : fields)
      for (double v : {nan, inf, -inf}) {
        const double keep = *f;
        *f = v;
        if (!track_common_check(&cam, 40)) wrong("a non-finite field is accepted");
        *f = keep;
      }
    for (double *f : {&cam.fx, &cam.fy}) {
      const double keep = *f;
      *f = 0.0;
      if (!track_common_check(&cam, 40)) wrong("a zero focal length is accepted");
      *f = -keep;
      if (track_common_check(&cam, 40)) wrong("a negative focal length is refused");
      *f = keep;
    }
    for (int model : {1, 4, 7, -1}) {
      cam.model = model;
      if (!track_common_check(&cam, 40)) wrong("a model outside {0, 2, 3, 5} is accepted");
    }
    cam.model = LFVIO_CAM_KANNALA_BRANDT;
    for (int N : {-1, 4097})
      if (!track_common_check(&cam, N)) wrong("num_points outside [0, 4096] is accepted");
  }
  // the routines alone, far outside what a pixel gives
  for (double th : {0.0, 1e-300, 0.5, 1e6, 1e15, 1e22, 3e38, 1e300, inf, nan}) {
    double s, c;
    kb_sincos(th, s, c);
    if (th <= 1e6 && std::fabs(s * s + c * c - 1.0) > 1e-9) wrong("sin^2 + cos^2");
  }
  std::printf("camera_kb walk: %ld rays, %ld beyond r_lim, %ld NaN rays, %d wrong\n", rays, fallbacks, nans, bad);
  return bad ? 1 : 0;
}
