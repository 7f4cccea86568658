// remap_plan_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/remap_plan.h and cam_project (camera_models.h, camera_atan.h) for a
// sanitizer build of the host side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/remap_plan_walk.cpp -o remap_plan_walk        (one line)
//   ./remap_plan_walk
// The 13 cameras of tests/test_camera_lift.py, every field a model does not read NaN (the inverse polynomial too, for the models
// that have none): proj_check and proj_cam; cam_project over a lattice of rays on the whole sphere and over the special rays (zeros,
// +-inf, NaN and a denormal in each component); the EQUIRECT and the PERSPECTIVE map at 33 x 17 and 64 x 48, every entry through
// remap_index / remap_offset for a 64 x 48 source in every encoding, and the nearest remap of a source image on the host with its
// reads checked against the image's own size — the host's copy of what k_remap_apply does, in bounds by the sanitizer's word; then
// every refusal of remap_project_check / remap_build_check / remap_apply_check, the rebuild decision and the launch geometry at the
// smallest and the largest size.  What the walk asserts is coarse (a ray inside the image projects into it again to 0.1 px for the
// models whose projection inverts the lift, offsets stay inside the source, the verdicts are the expected ones): the bits are
// tests/test_camera_project.py's and tests/test_remap_plan.py's business.  Exit code 1 when something is not as expected.
#include <cstdio>
#include <limits>
#include <vector>

#include "remap_plan.h"

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
static LfvioProjector projector(const LfvioCamera *cam) {
  const double inv[14] = {376.845565, 246.746504, 19.035187, 23.840497, 18.991943, 6.066253, 1.560387, 5.854280, 3.458320, -1.995166, -1.509264,
                          1.089614, 1.340245, 0.255323};
  LfvioProjector p;
  p.camera = cam;
  for (int i = 0; i < LFVIO_OCAM_INV_POLY_SIZE; i++) p.inv_poly[i] = cam->model == LFVIO_CAM_OCAM ? (i < 14 ? inv[i] : 0.0) : nan_;
  return p;
}

// cv::remap(..., INTER_NEAREST) on the host through remap_offset, every read checked against the source's size
static long gather(const std::vector<float> &mx, const std::vector<float> &my, const RemapGeom &g, const std::vector<unsigned char> &src,
                   std::vector<unsigned char> &out) {
  long inside = 0;
  out.assign(mx.size() * (size_t)g.bpp, 0xee);
  for (size_t p = 0; p < mx.size(); p++) {
    const int o = remap_offset(mx[p], my[p], g);
    if (o >= 0 && (size_t)o + (size_t)g.bpp > src.size()) wrong("-", "an offset behind the source image");
    for (int k = 0; k < g.bpp; k++) out[p * (size_t)g.bpp + k] = o < 0 ? 0 : src[(size_t)o + k];
    inside += o >= 0;
  }
  return inside;
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
  const int encodings[] = {LFVIO_IMG_MONO8, LFVIO_IMG_BGR8, LFVIO_IMG_RGB8, LFVIO_IMG_BGRA8, LFVIO_IMG_RGBA8, LFVIO_IMG_MONO16, LFVIO_IMG_MONO16_BE};
  const int SW = 64, SH = 48;
  KbCache cache;
  long rays = 0, nans = 0, entries = 0, inside = 0, back = 0;
  if (!proj_check(nullptr)) wrong("-", "a null projector is accepted");
  for (const Entry &q : cams) {
    LfvioCamera cam = q.cam;
    LfvioProjector proj = projector(&cam);
    if (proj_check(&proj)) wrong(q.name, "the projector is refused");
    const ProjCam pc = proj_cam(proj, &cache), fresh = proj_cam(proj);
    if (pc.t.model != cam.model || pc.t.theta_lim != fresh.t.theta_lim || pc.fx != fresh.fx) wrong(q.name, "proj_cam");
    // a lattice over the sphere and the special values in each component
    const double odd[] = {nan_, inf_, -inf_, 1e-310, -1e-310, 0.0, -0.0};
    std::vector<double> vals;
    for (int k = -6; k <= 6; k++) vals.push_back(0.37 * k);
    const size_t plain = vals.size();
    for (double v : odd) vals.push_back(v);
    for (size_t a = 0; a < vals.size(); a++)
      for (size_t b = 0; b < vals.size(); b++)
        for (size_t c = 0; c < vals.size(); c++) {
          if ((a >= plain) + (b >= plain) + (c >= plain) > 1) continue;
          const CamPixel p = cam_project(pc, vals[a], vals[b], vals[c]);
          rays++, nans += p.u != p.u || p.v != p.v;
        }
    // project(lift(pixel)) comes back for the models whose projection inverts the lift exactly enough: PINHOLE and MEI without
    // distortion, KANNALA_BRANDT away from the rim; OCam on its annulus to the fit of inv_poly (0.05 px)
    const bool inverts = pc.t.model == LFVIO_CAM_KANNALA_BRANDT || pc.t.model == LFVIO_CAM_OCAM || pc.t.no_distortion;
    for (int y = q.height / 4; y <= 3 * q.height / 4; y += 9)
      for (int x = q.width / 4; x <= 3 * q.width / 4; x += 9) {
        const CamRay P = cam_lift(pc.t, (float)x, (float)y);
        const CamPixel p = cam_project(pc, P.x, P.y, P.z);
        const double r = std::sqrt((x - cam.cx) * (x - cam.cx) + (y - cam.cy) * (y - cam.cy));
        if (pc.t.model == LFVIO_CAM_OCAM && (r < 200.0 || r > 420.0)) continue;  // (off the annulus the fit is not the calibration's business)
        if (inverts && !(std::fabs(p.u - x) <= 0.1 && std::fabs(p.v - y) <= 0.1)) wrong(q.name, "project(lift(pixel)) is not the pixel");
        back++;
      }
    // both kinds of map at two sizes; every entry through the index, the offset and the host's gather in every encoding
    const double s = (double)q.width / SW;  // the map of the full-size camera, gathered from a source s times smaller: offsets only
    for (int kind : {LFVIO_MAP_EQUIRECT, LFVIO_MAP_PERSPECTIVE})
      for (int size = 0; size < 2; size++) {
        const int W = size ? 64 : 33, H = size ? 48 : 17;
        const double f = W / 2.0, M[9] = {1.0 / f, 0.0, -1.0, 0.0, -1.0 / f, (H / 2.0) / f, 0.0, 0.0, cam.model == LFVIO_CAM_OCAM ? -1.0 : 1.0};
        std::vector<float> mx((size_t)W * H), my((size_t)W * H);
        for (int j = 0; j < H; j++)
          for (int i = 0; i < W; i++) {
            const RemapEntry e = remap_entry(pc, kind, W, H, M, i, j);
            mx[(size_t)j * W + i] = (float)(e.x / s), my[(size_t)j * W + i] = (float)(e.y / s);
            const int ix = remap_index(e.x);
            if (ix < -32768 || ix > 32767) wrong(q.name, "remap_index outside a short");
          }
        entries += (long)mx.size();
        for (int enc : encodings)
          for (int pad : {0, 5}) {
            const LfvioImageFormat fmt = {enc, pad ? SW * imgfmt_bpp(enc) + pad : 0};
            if (remap_apply_check(&fmt, SW, SH, (const unsigned char *)"", (const unsigned char *)"")) wrong(q.name, "a format of the table is refused");
            const RemapGeom g = remap_geom(fmt, SW, SH);
            std::vector<unsigned char> src(imgfmt_bytes(fmt, SW, SH)), out;
            for (size_t k = 0; k < src.size(); k++) src[k] = (unsigned char)(1 + k % 251);
            inside += gather(mx, my, g, src, out);
            if (out.size() != (size_t)W * H * (size_t)g.bpp) wrong(q.name, "the output's size");
          }
      }
    // the refusals
    const double P3[3] = {0.1, 0.2, 1.0};
    double px2[2];
    float fx_ = 0.0f;
    if (remap_project_check(&proj, 1, P3, px2) || remap_project_check(&proj, 0, nullptr, nullptr)) wrong(q.name, "a valid projection is refused");
    if (!remap_project_check(&proj, -1, P3, px2) || !remap_project_check(&proj, REMAP_MAX_POINTS + 1, P3, px2) || !remap_project_check(&proj, 1, nullptr, px2) ||
        !remap_project_check(&proj, 1, P3, nullptr) || !remap_project_check(nullptr, 1, P3, px2))
      wrong(q.name, "remap_project_check");
    LfvioRemapIn in = {&proj, LFVIO_MAP_PERSPECTIVE, 33, 17, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
    if (remap_build_check(&in, &fx_, &fx_) || remap_build_check(&in, nullptr, nullptr)) wrong(q.name, "a valid build is refused");
    if (!remap_build_check(&in, &fx_, nullptr) || !remap_build_check(&in, nullptr, &fx_) || !remap_build_check(nullptr, &fx_, &fx_)) wrong(q.name, "map_x / map_y");
    for (int k = 0; k < 9; k++) {
      const double keep = in.M[k];
      in.M[k] = k % 2 ? nan_ : inf_;
      if (!remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "a non-finite M entry is accepted");
      in.kind = LFVIO_MAP_EQUIRECT;
      if (remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "EQUIRECT looks at M");
      in.kind = LFVIO_MAP_PERSPECTIVE, in.M[k] = keep;
    }
    for (int kind : {-1, 2, 7}) {
      in.kind = kind;
      if (!remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "an unknown kind is accepted");
    }
    in.kind = LFVIO_MAP_EQUIRECT;
    for (int side : {15, 8193, 0, -1}) {
      in.width = side;
      if (!remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "a width outside [16, 8192] is accepted");
      in.width = 33, in.height = side;
      if (!remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "a height outside [16, 8192] is accepted");
      in.height = 17;
    }
    in.width = in.height = 8192;
    if (remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "8192 x 8192 is refused");
    if (cam.model == LFVIO_CAM_OCAM)
      for (int k : {0, 13, 19}) {
        const double keep = proj.inv_poly[k];
        proj.inv_poly[k] = k ? nan_ : -inf_;
        if (!proj_check(&proj) || !remap_build_check(&in, &fx_, &fx_) || !remap_project_check(&proj, 1, P3, px2)) wrong(q.name, "a non-finite inv_poly entry is accepted");
        proj.inv_poly[k] = keep;
      }
    proj.camera = nullptr;
    if (!proj_check(&proj) || !remap_build_check(&in, &fx_, &fx_)) wrong(q.name, "a null camera is accepted");
    proj.camera = &cam, cam.model = 4;
    if (!proj_check(&proj)) wrong(q.name, "model 4 is accepted");
  }
  // the apply's checks, the rebuild decision, the geometry
  const unsigned char byte = 0;
  const LfvioImageFormat bgr = {LFVIO_IMG_BGR8, 0}, bad_code = {1, 0}, short_step = {LFVIO_IMG_BGR8, 191}, long_step = {LFVIO_IMG_BGR8, 65537};
  if (remap_apply_check(&bgr, 64, 48, &byte, &byte) || remap_apply_check(nullptr, 64, 48, &byte, &byte)) wrong("-", "a valid apply is refused");
  if (!remap_apply_check(&bgr, 64, 48, nullptr, &byte) || !remap_apply_check(&bgr, 64, 48, &byte, nullptr) || !remap_apply_check(&bad_code, 64, 48, &byte, &byte) ||
      !remap_apply_check(&short_step, 64, 48, &byte, &byte) || !remap_apply_check(&long_step, 64, 48, &byte, &byte) || !remap_apply_check(&bgr, 15, 48, &byte, &byte) ||
      !remap_apply_check(&bgr, 64, 8193, &byte, &byte))
    wrong("-", "remap_apply_check");
  RemapResident r;
  const RemapGeom g0 = remap_geom(bgr, 1280, 960);
  if (!remap_needs_index(r, g0)) wrong("-", "no integer map, and none asked for");
  r.indexed = true, r.geom = g0;
  const LfvioImageFormat same_step = {LFVIO_IMG_BGR8, 3840}, padded = {LFVIO_IMG_BGR8, 3844}, mono = {LFVIO_IMG_MONO8, 0};
  if (remap_needs_index(r, g0) || remap_needs_index(r, remap_geom(same_step, 1280, 960))) wrong("-", "a rebuild for the same source");
  if (!remap_needs_index(r, remap_geom(padded, 1280, 960)) || !remap_needs_index(r, remap_geom(mono, 1280, 960)) || !remap_needs_index(r, remap_geom(bgr, 1280, 961)) ||
      !remap_needs_index(r, remap_geom(bgr, 1279, 960)))
    wrong("-", "no rebuild for another source");
  for (int side : {16, 33, 8192}) {
    const RemapGrid g = remap_build_grid(side, side);
    const size_t n = (size_t)side * side;
    if ((size_t)g.x * REMAP_TILE_W < (size_t)side || (size_t)g.y * REMAP_TILE_H < (size_t)side) wrong("-", "the build's grid does not cover the image");
    if ((size_t)remap_apply_blocks(n) * REMAP_THREADS * REMAP_RUN < n || (size_t)(remap_apply_blocks(n) - 1) * REMAP_THREADS * REMAP_RUN >= n) wrong("-", "the apply's grid");
  }
  if (remap_project_blocks(REMAP_MAX_POINTS) * REMAP_PROJECT_THREADS < (unsigned)REMAP_MAX_POINTS || remap_project_blocks(1) != 1) wrong("-", "the projection's grid");
  const float idx[] = {-0.5f, 0.5f, 1.5f, 32766.5f, 32767.5f, 1e10f, -1e10f, (float)inf_, (float)-inf_, (float)nan_, -0.0f};
  const int want[] = {0, 0, 2, 32766, 32767, 32767, -32768, 32767, -32768, -32768, 0};
  for (size_t k = 0; k < sizeof idx / sizeof idx[0]; k++)
    if (remap_index(idx[k]) != want[k]) wrong("-", "remap_index");
  if (nans == 0 || nans == rays) wrong("-", "the special rays gave no NaN, or nothing else");
  if (inside == 0 || back == 0) wrong("-", "no map entry inside the source, or no round trip");
  std::printf("remap_plan walk: %d cameras, %ld rays (%ld NaN pixels), %ld round trips, %ld map entries, %ld gathered pixels, %d wrong\n",
              (int)(sizeof cams / sizeof cams[0]), rays, nans, back, entries, inside, bad);
  return bad ? 1 : 0;
}
