// camera_models_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/camera_models.h for a sanitizer build of the host side (no HIP, no
// GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/camera_models_walk.cpp -o camera_models_walk        (one line)
//   ./camera_models_walk
// The 13 cameras of tests/test_camera_lift.py (PAL, SKEW, the five of tests/camera_ref.py, the six of tests/kb_ref.py), every field a
// model does not read NaN: track_camera_check and track_cam, then cam_lift, cam_bearing and cam_undistorted over a pixel grid that
// covers the image and 50 px beyond it, the centre, and +-0, +-3e38, +-inf, NaN and a denormal in either coordinate and in both; then
// every field the model reads made non-finite, each alone, fx and fy zero and negative, the refused models and a null camera.  What
// the walk asserts is coarse (a pixel of the grid gives a unit bearing to 1e-12, un_pts_3d is that bearing rounded to float, the
// verdicts are the expected ones): the bits are tests/test_camera_lift.py's business.  Exit code 1 when something is not as expected.
#include <cstdio>
#include <limits>
#include <vector>

#include "camera_models.h"

static int bad = 0;
static void wrong(const char *cam, const char *what) { std::printf("WRONG: %s: %s\n", cam, what), bad++; }

static const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf_ = std::numeric_limits<double>::infinity();

struct Entry {
  const char *name;
  int width, height;
  LfvioCamera cam;
};

static LfvioCamera blank(int model, double cx, double cy) {  // everything else NaN: a field the header must not read
  LfvioCamera k;
  k.model = model, k.cx = cx, k.cy = cy, k.c = k.d = k.e = k.fx = k.fy = k.k1 = k.k2 = k.p1 = k.p2 = k.xi = nan_;
  for (double &p : k.poly) p = nan_;
  return k;
}
static Entry ocam(const char *name, double cx, double cy, double c, double d, double e) {
  LfvioCamera k = blank(LFVIO_CAM_OCAM, cx, cy);
  const double poly[5] = {-2.445239e+02, 0.0, 1.748610e-03, -1.757770e-06, 4.475965e-09};
  k.c = c, k.d = d, k.e = e;
  for (int i = 0; i < 5; i++) k.poly[i] = poly[i];
  return {name, 1280, 960, k};
}
static Entry plane(const char *name, int model, double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double xi) {
  LfvioCamera k = blank(model, cx, cy);
  k.fx = fx, k.fy = fy, k.k1 = k1, k.k2 = k2, k.p1 = p1, k.p2 = p2;
  if (model == LFVIO_CAM_MEI) k.xi = xi;
  return {name, 752, 480, k};
}
static Entry kb(const char *name, int w, int h, double k2, double k3, double k4, double k5, double mu, double mv, double u0, double v0) {
  LfvioCamera k = blank(LFVIO_CAM_KANNALA_BRANDT, u0, v0);
  k.fx = mu, k.fy = mv, k.poly[0] = k2, k.poly[1] = k3, k.poly[2] = k4, k.poly[3] = k5;
  return {name, w, h, k};
}

int main() {
  const double cla[4] = {472.2863830700696, 470.83759684346785, 368.8316828103749, 232.23688706965652};
  const Entry cams[] = {
      ocam("PAL", 645.107791, 486.025172, 1.0, 0.0, 0.0),
      ocam("SKEW", 640.5, 479.25, 1.0007, -0.0023, 0.0031),
      plane("EUROC", LFVIO_CAM_PINHOLE, 461.6, 460.3, 363.0, 248.1, -0.2917, 0.08228, 5.333e-05, -1.578e-04, nan_),
      plane("MV3DM", LFVIO_CAM_MEI, 1115.0, 1114.0, 367.2, 238.5, 0.07145, 0.5059, 4.727e-05, -5.492e-04, 2.057),
      plane("EUROC_ND", LFVIO_CAM_PINHOLE, 461.6, 460.3, 363.0, 248.1, 0.0, 0.0, 0.0, 0.0, nan_),
      plane("MV3DM_ND", LFVIO_CAM_MEI, 1115.0, 1114.0, 367.2, 238.5, 0.0, 0.0, 0.0, 0.0, 2.057),
      plane("MEI_XI1", LFVIO_CAM_MEI, 1115.0, 1114.0, 367.2, 238.5, 0.07145, 0.5059, 4.727e-05, -5.492e-04, 1.0),
      kb("TUM", 512, 512, 0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182, 190.97847715128717,
         190.9733070521226, 254.93170605935475, 256.8974428996504),
      kb("CLA", 752, 480, -0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.02008469575876223, cla[0], cla[1], cla[2], cla[3]),
      kb("RSFISH", 640, 480, 1.7280355035195181e-02, -2.5505200860040985e-02, 2.2621441637715487e-02, -7.3355871719731113e-03,
         2.7723712054408202e+02, 2.7699784668734617e+02, 3.3625356873985868e+02, 2.3603924727453901e+02),
      kb("KB_K5_0", 752, 480, -0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.0, cla[0], cla[1], cla[2], cla[3]),
      kb("KB_K45_0", 752, 480, -0.005740195474458931, 0.02878252863739417, 0.0, 0.0, cla[0], cla[1], cla[2], cla[3]),
      kb("KB_IDEAL", 752, 480, 0.0, 0.0, 0.0, 0.0, cla[0], cla[1], cla[2], cla[3]),
  };
  KbCache cache;
  long rays = 0, nans = 0;
  int seen_nd = 0, seen_xi1 = 0;
  if (!track_camera_check(nullptr)) wrong("-", "a null camera is accepted");
  for (const Entry &q : cams) {
    LfvioCamera cam = q.cam;
    if (track_camera_check(&cam)) wrong(q.name, "the camera is refused");
    const TrackCam t = track_cam(cam, &cache), fresh = track_cam(cam);
    if (t.model != cam.model || t.theta_lim != fresh.theta_lim || t.r_lim != fresh.r_lim) wrong(q.name, "track_cam");
    seen_nd += t.no_distortion, seen_xi1 += t.xi == 1.0;
    const size_t grid_x = (size_t)(q.width + 100) / 7 + 1, grid_y = (size_t)(q.height + 100) / 7 + 1;
    std::vector<float> xs, ys;
    for (int x = -50; x <= q.width + 50; x += 7) xs.push_back((float)x + 0.25f);
    for (int y = -50; y <= q.height + 50; y += 7) ys.push_back((float)y + 0.5f);
    if (xs.size() != grid_x || ys.size() != grid_y) wrong(q.name, "the grid");
    const float odd[] = {(float)nan_, (float)inf_, (float)-inf_, 3e38f, -3e38f, 0.0f, -0.0f, 1e-40f};
    xs.push_back((float)cam.cx), ys.push_back((float)cam.cy);
    for (float v : odd) xs.push_back(v), ys.push_back(v);
    for (size_t i = 0; i < xs.size(); i++)
      for (size_t j = 0; j < ys.size(); j++) {
        const float px = xs[i], py = ys[j];
        const CamRay P = cam_lift(t, px, py);
        double b[3];
        cam_bearing(t, px, py, b);
        const CamUndistorted u = cam_undistorted(t, px, py);
        rays++;
        const bool ordinary = i <= grid_x && j <= grid_y;  // the grid and the centre
        if (b[0] != b[0] || b[1] != b[1] || b[2] != b[2]) {
          nans++;
          if (ordinary) wrong(q.name, "a NaN bearing from an ordinary pixel");
          continue;
        }
        if (ordinary && !(std::fabs(std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) - 1.0) <= 1e-12)) wrong(q.name, "a bearing that is no unit vector");
        if (u.bx != (float)b[0] || u.by != (float)b[1] || u.bz != (float)b[2]) wrong(q.name, "un_pts_3d is not the bearing as float");
        if (ordinary && P.z != 0.0 && u.ux != (float)(P.x / P.z)) wrong(q.name, "un_pts");
      }
    // every field the model reads, non-finite, each alone; what it does not read is NaN already
    std::vector<double *> fields;
    if (cam.model != LFVIO_CAM_OCAM) fields = {&cam.cx, &cam.cy, &cam.fx, &cam.fy};
    if (cam.model == LFVIO_CAM_KANNALA_BRANDT) fields.insert(fields.end(), {&cam.poly[0], &cam.poly[1], &cam.poly[2], &cam.poly[3]});
    if (cam.model == LFVIO_CAM_PINHOLE || cam.model == LFVIO_CAM_MEI) fields.insert(fields.end(), {&cam.k1, &cam.k2, &cam.p1, &cam.p2});
    if (cam.model == LFVIO_CAM_MEI) fields.push_back(&cam.xi);
    for (double *f : fields)
      for (double v : {nan_, inf_, -inf_}) {
        const double keep = *f;
        *f = v;
        if (!track_camera_check(&cam)) wrong(q.name, "a non-finite field is accepted");
        *f = keep;
      }
    if (cam.model != LFVIO_CAM_OCAM)
      for (double *f : {&cam.fx, &cam.fy}) {
        const double keep = *f;
        *f = 0.0;
        if (!track_camera_check(&cam)) wrong(q.name, "a zero focal length is accepted");
        *f = -keep;
        if (track_camera_check(&cam)) wrong(q.name, "a negative focal length is refused");
        *f = keep;
      }
    for (int model : {1, 4, 7, -1}) {
      cam.model = model;
      if (!track_camera_check(&cam)) wrong(q.name, "a model outside {0, 2, 3, 5} is accepted");
    }
  }
  if (seen_nd != 2 || seen_xi1 != 1) wrong("-", "no_distortion or xi == 1.0 was not met where expected");
  if (nans == 0 || nans == rays) wrong("-", "the special pixels gave no NaN, or nothing else");
  std::printf("camera_models walk: %d cameras, %ld rays, %ld NaN bearings, %d wrong\n", (int)(sizeof cams / sizeof cams[0]), rays, nans, bad);
  return bad ? 1 : 0;
}
