// camera_models.h — everything about a camera model, in one header that the host and the device both compile: the camera as the
// kernels take it (TrackCam, formed by track_cam on the host), the argument check of an LfvioCamera (track_camera_check) and the lift
// of a pixel for the four models of include/lfvio.h:
//   LFVIO_CAM_OCAM             OCAMCamera::liftProjective (camera_model/src/camera_models/ScaramuzzaCamera.cc:623-645)
//   LFVIO_CAM_PINHOLE          PinholeCamera::liftProjective (PinholeCamera.cc:450-510)
//   LFVIO_CAM_MEI              CataCamera::liftProjective (CataCamera.cc:556-626)
//   LFVIO_CAM_KANNALA_BRANDT   EquidistantCamera::liftProjective (EquidistantCamera.cc:428-442), restated in camera_kb.h
//   LFVIO_CAM_EQUIRECT         the expanded image of LFVIO_MAP_EQUIRECT: GetremapMat's ray (pointcloud_image_fusion.cpp:93-101) at a float
//                              pixel — the lift only (proj_check refuses it); numpy: tests/equirect_ref.py
// and what every model shares behind the lift: the norm, the unit bearing of rejectWithF and the two float outputs of
// undistortedPoints.  The specification is in include/lfvio.h and, as numpy, in tests/track_ref.py (OCam), tests/camera_ref.py
// (PINHOLE, MEI) and tests/kb_ref.py (KANNALA_BRANDT).  The other way — spaceToPlane of the four models, cam_project over the
// arctangent of camera_atan.h, with ProjCam / proj_cam / proj_check — is at the end of the file (numpy: tests/project_ref.py; held to
// it by tests/test_camera_project.py; walked under the CPU sanitizers by tests/tools/remap_plan_walk.cpp).
//
// Plain C++ when compiled without hipcc (nothing from HIP, dev_math.h or kernels_twoview.h); under hipcc the per-pixel functions are
// __host__ __device__ (KB_HD of camera_kb.h), as image_format.h's pixel conversions are.  kernels_track.h calls them from the kernels,
// track_plan.h includes this file for the host side, and tests/test_camera_lift.py compiles it alone with g++ and holds every lift to
// its numpy text bit for bit; tests/tools/camera_models_walk.cpp walks it under the CPU sanitizers.
//
// Every lift is written operation by operation and every user compiles with -ffp-contract=off: each product and sum is rounded on
// its own, grouped as include/lfvio.h states it.  The norm is sqrt((x x + y y) + z z), left to right as tv_residual forms its norms;
// Eigen's own reduction may order the terms differently (the reference does not build here, so the two were never compared).  A
// camera's model is the same in every thread of a workgroup (a kernel argument, or the slot's camera in the batched route), so the
// branches on it are uniform, and no trip count depends on a pixel.
#pragma once
#include <cmath>

#include "../../include/lfvio.h"
#include "camera_atan.h"
#include "camera_kb.h"

struct TrackCam {  // a kernel argument, by value; the members a model does not use are zero
  double cx, cy, c, d, e, inv_scale, poly[5];          // OCam
  double inv11, inv13, inv22, inv23, k1, k2, p1, p2, xi;  // PINHOLE and MEI (xi: MEI), PinholeCamera.cc:281-289
  int model, no_distortion;
  double theta_lim, r_lim;  // KANNALA_BRANDT (camera_kb.h), with inv11 .. inv23 and k2 .. k5 in poly[0 .. 3]
  // EQUIRECT: the expanded image's width and height in cx and cy, nothing else
};

// On the host, in double, once per call (inv_scale: ScaramuzzaCamera.cc:197).  LfvioCamera's fx .. xi are read only for PINHOLE and
// MEI, its c, d, e, poly only for OCam; KANNALA_BRANDT reads cx, cy, fx, fy and poly[0 .. 3], EQUIRECT fx and fy: callers may leave the
// others indeterminate.
// kb: where a KANNALA_BRANDT camera's constants are kept from one call to the next (nullptr: formed anew); no other model looks at it.
inline TrackCam track_cam(const LfvioCamera &k, KbCache *kb = nullptr) {
  TrackCam t = {};
  t.model = k.model;
  if (k.model == LFVIO_CAM_EQUIRECT) {
    t.cx = k.fx, t.cy = k.fy;
    return t;
  }
  t.cx = k.cx, t.cy = k.cy;
  if (k.model == LFVIO_CAM_OCAM) {
    t.c = k.c, t.d = k.d, t.e = k.e;
    t.inv_scale = 1.0 / (k.c - k.d * k.e);
    for (int i = 0; i < 5; i++) t.poly[i] = k.poly[i];
    return t;
  }
  t.inv11 = 1.0 / k.fx, t.inv13 = -k.cx / k.fx, t.inv22 = 1.0 / k.fy, t.inv23 = -k.cy / k.fy;
  if (k.model == LFVIO_CAM_KANNALA_BRANDT) {
    const double key[8] = {k.cx, k.cy, k.fx, k.fy, k.poly[0], k.poly[1], k.poly[2], k.poly[3]};
    KbCache once;
    const KbConstants &c = (kb ? *kb : once).get(key);
    for (int i = 0; i < 4; i++) t.poly[i] = k.poly[i];
    t.theta_lim = c.theta_lim, t.r_lim = c.r_lim;
    return t;
  }
  t.k1 = k.k1, t.k2 = k.k2, t.p1 = k.p1, t.p2 = k.p2;
  t.no_distortion = k.k1 == 0.0 && k.k2 == 0.0 && k.p1 == 0.0 && k.p2 == 0.0;
  if (k.model == LFVIO_CAM_MEI) t.xi = k.xi;
  return t;
}

constexpr int CAM_EQUIRECT_MIN_SIDE = 16, CAM_EQUIRECT_MAX_SIDE = 8192;  // (IMGFMT_MIN_SIDE, IMGFMT_MAX_SIDE of image_format.h)

// nullptr, or what is wrong with the camera.  v: the fields the model reads besides MEI's xi (OCam's are not judged)
inline const char *track_camera_check(const LfvioCamera *cam) {
  if (!cam) return "lfvio_track: null camera";
  if (cam->model != LFVIO_CAM_OCAM && cam->model != LFVIO_CAM_PINHOLE && cam->model != LFVIO_CAM_MEI && cam->model != LFVIO_CAM_KANNALA_BRANDT &&
      cam->model != LFVIO_CAM_EQUIRECT)
    return "lfvio_track: a camera model other than LFVIO_CAM_OCAM, LFVIO_CAM_PINHOLE, LFVIO_CAM_MEI, LFVIO_CAM_KANNALA_BRANDT and LFVIO_CAM_EQUIRECT";
  if (cam->model == LFVIO_CAM_OCAM) return nullptr;
  if (cam->model == LFVIO_CAM_EQUIRECT) {  // fx, fy: the expanded image's width and height (a NaN fails every comparison)
    const double side[2] = {cam->fx, cam->fy};
    for (double x : side)
      if (!(x >= (double)CAM_EQUIRECT_MIN_SIDE && x <= (double)CAM_EQUIRECT_MAX_SIDE) || x != std::floor(x))
        return "lfvio_track: LFVIO_CAM_EQUIRECT with fx or fy (the image's width and height) not an integer in [16, 8192]";
    return nullptr;
  }
  const bool kb = cam->model == LFVIO_CAM_KANNALA_BRANDT;
  const double v[8] = {cam->cx, cam->cy, cam->fx, cam->fy, kb ? cam->poly[0] : cam->k1, kb ? cam->poly[1] : cam->k2,
                       kb ? cam->poly[2] : cam->p1, kb ? cam->poly[3] : cam->p2};
  for (double x : v)
    if (!std::isfinite(x)) return "lfvio_track: a non-finite camera parameter";
  if (cam->fx == 0.0 || cam->fy == 0.0) return "lfvio_track: fx or fy is zero";
  if (cam->model == LFVIO_CAM_MEI && !std::isfinite(cam->xi)) return "lfvio_track: a non-finite xi";
  return nullptr;
}

// ---- per pixel
struct CamRay { double x, y, z; };

// PinholeCamera::distortion (PinholeCamera.cc:646-662; CataCamera's is the same text): grouped as include/lfvio.h states it
KB_HD void cam_distortion(const TrackCam &cam, double x, double y, double &dx, double &dy) {
  const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2;
  const double rad = cam.k1 * rho2 + (cam.k2 * rho2) * rho2;
  dx = (x * rad + (2.0 * cam.p1) * mxy) + cam.p2 * (rho2 + 2.0 * mx2);
  dy = (y * rad + (2.0 * cam.p2) * mxy) + cam.p1 * (rho2 + 2.0 * my2);
}

// PinholeCamera::liftProjective (:450-510): the normalised plane and the recursive distortion model, n = 8 evaluations, and z = 1.
// CataCamera's (CataCamera.cc:562-612) is the same text up to its z.
KB_HD CamRay cam_lift_pinhole(const TrackCam &cam, float px, float py) {
  const double mx_d = cam.inv11 * (double)px + cam.inv13, my_d = cam.inv22 * (double)py + cam.inv23;
  if (cam.no_distortion) return {mx_d, my_d, 1.0};
  double mx_u = mx_d, my_u = my_d;
  for (int i = 0; i < 8; i++) {
    double dx, dy;
    cam_distortion(cam, mx_u, my_u, dx, dy);
    mx_u = mx_d - dx, my_u = my_d - dy;
  }
  return {mx_u, my_u, 1.0};
}

// CataCamera::liftProjective (:556-626)
KB_HD CamRay cam_lift_mei(const TrackCam &cam, float px, float py) {
  const CamRay P = cam_lift_pinhole(cam, px, py);
  const double mx_u = P.x, my_u = P.y;
  if (cam.xi == 1.0) return {mx_u, my_u, ((1.0 - mx_u * mx_u) - my_u * my_u) / 2.0};  // :618
  const double rho2 = mx_u * mx_u + my_u * my_u;
  return {mx_u, my_u, 1.0 - (cam.xi * (rho2 + 1.0)) / (cam.xi + sqrt(1.0 + (1.0 - cam.xi * cam.xi) * rho2))};  // :624
}

// LFVIO_CAM_EQUIRECT: remap_ray's text (remap_plan.h, LFVIO_MAP_EQUIRECT) with the float pixel in place of (i, j); cx, cy: width, height
KB_HD CamRay cam_lift_equirect(const TrackCam &cam, float px, float py) {
  constexpr double PI = 3.14159265358979323846;
  const double lon = ((double)px / cam.cx - 0.5) * (2.0 * PI);
  const double lat = -(((double)py / cam.cy - 0.5) * PI);
  double slon, clon, slat, clat;
  kb_sincos(lon, slon, clon);
  kb_sincos(lat, slat, clat);
  return {clat * slon, clat * clon, slat};
}

// liftProjective of the pixel (px, py).  KANNALA_BRANDT: as camera_kb.h restates it; OCAMCamera::liftProjective (:623-645):
KB_HD CamRay cam_lift(const TrackCam &cam, float px, float py) {
  if (cam.model == LFVIO_CAM_PINHOLE) return cam_lift_pinhole(cam, px, py);
  if (cam.model == LFVIO_CAM_MEI) return cam_lift_mei(cam, px, py);
  if (cam.model == LFVIO_CAM_KANNALA_BRANDT) {
    CamRay P;
    kb_lift_pixel(cam.inv11, cam.inv13, cam.inv22, cam.inv23, cam.poly, cam.theta_lim, cam.r_lim, px, py, P.x, P.y, P.z);
    return P;
  }
  if (cam.model == LFVIO_CAM_EQUIRECT) return cam_lift_equirect(cam, px, py);
  const double x = (double)px - cam.cx, y = (double)py - cam.cy;  // :627
  const double xa = cam.inv_scale * (x - cam.d * y), ya = cam.inv_scale * (-cam.e * x + cam.c * y);  // :631-632
  const double phi = sqrt(xa * xa + ya * ya);
  double p = 1.0, z = 0.0;
  for (int i = 0; i < 5; i++) {  // :638-642
    z += p * cam.poly[i];
    p *= phi;
  }
  return {xa, ya, -z};  // :644
}

KB_HD double cam_norm(CamRay P) { return sqrt((P.x * P.x + P.y * P.y) + P.z * P.z); }

// rejectWithF's unit bearing of a pixel (feature_tracker.cpp:343, :353), three doubles
KB_HD void cam_bearing(const TrackCam &cam, float px, float py, double *b) {
  const CamRay P = cam_lift(cam, px, py);
  const double n = cam_norm(P);
  b[0] = P.x / n, b[1] = P.y / n, b[2] = P.z / n;
}

// undistortedPoints' two outputs for a pixel: un_pts (:454) and un_pts_3d (:455), the quotients in double, rounded to float once
struct CamUndistorted { float ux, uy, bx, by, bz; };
KB_HD CamUndistorted cam_undistorted(const TrackCam &cam, float px, float py) {
  const CamRay Q = cam_lift(cam, px, py);
  const double n = cam_norm(Q);
  return {(float)(Q.x / Q.z), (float)(Q.y / Q.z), (float)(Q.x / n), (float)(Q.y / n), (float)(Q.z / n)};
}

// ---- the other way: spaceToPlane of the four models (include/lfvio.h, lfvio_cam_project)
//   LFVIO_CAM_OCAM             OCAMCamera::spaceToPlane (ScaramuzzaCamera.cc:654-674)
//   LFVIO_CAM_PINHOLE          PinholeCamera::spaceToPlane (PinholeCamera.cc:520-542)
//   LFVIO_CAM_MEI              CataCamera::spaceToPlane (CataCamera.cc:636-659)
//   LFVIO_CAM_KANNALA_BRANDT   EquidistantCamera::spaceToPlane (EquidistantCamera.cc:451-461), its mathematics in a text of this library's
// The specification as numpy is tests/project_ref.py; tests/test_camera_project.py holds cam_project to it bit for bit.
// ProjCam is the TrackCam of the lifts plus what only the projection reads; proj_cam forms it on the host.  TrackCam, track_cam
// and the lifts above are what they were: the kernels that take them keep their instructions.
constexpr int CAM_INV_POLY = LFVIO_OCAM_INV_POLY_SIZE;
struct ProjCam {  // a kernel argument, by value
  TrackCam t;
  double fx, fy;                  // as given (PINHOLE, MEI, KANNALA_BRANDT); OCam: zero
  double inv_poly[CAM_INV_POLY];  // OCam; the other models: zero
};

inline ProjCam proj_cam(const LfvioProjector &p, KbCache *kb = nullptr) {
  ProjCam q = {};
  q.t = track_cam(*p.camera, kb);
  if (p.camera->model == LFVIO_CAM_OCAM)
    for (int i = 0; i < CAM_INV_POLY; i++) q.inv_poly[i] = p.inv_poly[i];
  else
    q.fx = p.camera->fx, q.fy = p.camera->fy;
  return q;
}

// nullptr, or what is wrong with the projector: its camera as track_camera_check judges it — but no LFVIO_CAM_EQUIRECT, which has no
// projection here — and, for OCam, a finite inverse polynomial
inline const char *proj_check(const LfvioProjector *p) {
  if (!p) return "lfvio_cam_project: null projector";
  if (const char *why = track_camera_check(p->camera)) return why;
  if (p->camera->model == LFVIO_CAM_EQUIRECT)  // (cam_project would fall through to the OCam branch)
    return "lfvio_cam_project: LFVIO_CAM_EQUIRECT has the lift only (the projection is LFVIO_FUSE_EQUIRECT of lfvio_cloud_fuse)";
  if (p->camera->model == LFVIO_CAM_OCAM)
    for (double x : p->inv_poly)
      if (!std::isfinite(x)) return "lfvio_cam_project: a non-finite inv_poly entry";
  return nullptr;
}

struct CamPixel { double u, v; };

// PINHOLE (:520-542) and, with z = Z + xi |P|, MEI (:636-659)
KB_HD CamPixel cam_project_plane(const ProjCam &cam, double X, double Y, double z) {
  double x = X / z, y = Y / z;
  if (!cam.t.no_distortion) {
    double dx, dy;
    cam_distortion(cam.t, x, y, dx, dy);
    x += dx, y += dy;
  }
  return {cam.fx * x + cam.t.cx, cam.fy * y + cam.t.cy};
}

// KANNALA_BRANDT: theta in [0, pi] with tangent rxy / Z from cam_atan, (cos phi, sin phi) = (X, Y) / rxy, r = F(theta).
// Stated deviations from the reference's text (acos(Z / |P|), atan2(Y, X), cos, sin): theta from the arctangent of rxy / Z
// (the same angle; better conditioned near the axis than the arc cosine); X / rxy, Y / rxy in place of cos(atan2(Y, X)),
// sin(atan2(Y, X)); rxy < 1e-10 gives phi = 0 as the lift's r < 1e-10 does, where the reference's atan2 still follows (X, Y);
// the zero vector is NaN here as there (0 / 0).
KB_HD CamPixel cam_project_kb(const ProjCam &cam, double X, double Y, double Z) {
  constexpr double PI_HI = 3.14159265358979311600e+00, PI_LO = 1.22464679914735317723e-16, PIO2 = 1.57079632679489655800e+00;
  const double rxy = sqrt(X * X + Y * Y);
  const double q = rxy / Z, a = cam_atan(q);
  // Z > 0: atan(q); Z < 0: pi + atan(q), q < 0; Z == 0: pi / 2 off the axis, 0 / 0 = NaN on it; a NaN Z: NaN (q)
  const double theta = Z > 0.0 ? a : Z < 0.0 ? PI_HI + (a + PI_LO) : (Z == 0.0 && rxy > 0.0) ? PIO2 : q;
  const bool tiny = rxy < 1e-10;
  const double cphi = tiny ? 1.0 : X / rxy, sphi = tiny ? 0.0 : Y / rxy;
  const double r = kb_f(cam.t.poly, theta);
  return {cam.fx * (r * cphi) + cam.t.cx, cam.fy * (r * sphi) + cam.t.cy};
}

// spaceToPlane of the point (X, Y, Z).  OCam (:654-674): theta = atan(-Z / n) stands for the reference's atan2(-Z, n), n >= 0 — at
// n == 0 the reference's pixel is NaN too (0 * inf), so the deviation is of the text, not of the value — and the inverse polynomial
// is the reference's running power over all SCARAMUZZA_INV_POLY_SIZE = 20 terms, not Horner.
KB_HD CamPixel cam_project(const ProjCam &cam, double X, double Y, double Z) {
  if (cam.t.model == LFVIO_CAM_PINHOLE) return cam_project_plane(cam, X, Y, Z);
  if (cam.t.model == LFVIO_CAM_MEI) return cam_project_plane(cam, X, Y, Z + cam.t.xi * cam_norm({X, Y, Z}));
  if (cam.t.model == LFVIO_CAM_KANNALA_BRANDT) return cam_project_kb(cam, X, Y, Z);
  const double n = sqrt(X * X + Y * Y);
  const double theta = cam_atan(-Z / n);
  double rho = 0.0, t = 1.0;
  for (int i = 0; i < CAM_INV_POLY; i++) {
    rho += t * cam.inv_poly[i];
    t *= theta;
  }
  const double inv = 1.0 / n;
  const double xn = (X * inv) * rho, yn = (Y * inv) * rho;
  return {(xn * cam.t.c + yn * cam.t.d) + cam.t.cx, (xn * cam.t.e + yn) + cam.t.cy};
}
