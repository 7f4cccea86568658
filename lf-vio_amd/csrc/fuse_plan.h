// fuse_plan.h — the host-side plan of lfvio_cloud_fuse (include/lfvio.h): the argument check, the read of a float32 field
// from a point's bytes in either byte order, fuse_point — one lidar point into the camera frame, through the range gate and onto its
// pixel of the equirectangular image (the inverse of remap_ray's EQUIRECT) or of the camera's own (cam_project) — and the launch
// geometry.  Plain C++ (no HIP); the per-point functions are host-and-device functions under hipcc (KB_HD of camera_kb.h), so
// k_fuse_project (kernels_fuse.h) and the host run the same text.  fuse.inc uses it, tests/test_fuse_plan.py compiles it alone with
// g++ and holds it to tests/fuse_ref.py bit for bit, tests/tools/fuse_plan_walk.cpp walks it under the CPU sanitizers.
//
// The reference's text (pointcloud_image_fusion_node.cpp:92-115) normalises the point and takes atan2(x, y) and asin(z); here the
// longitude is the angle of atan2(X, Y) built on cam_atan as cam_project_kb builds its theta, and the latitude is cam_atan(Z / nxy):
// the same angles in + - * / sqrt alone, every operation rounded on its own (-ffp-contract=off), no libm call.
#pragma once
#include <cmath>
#include <cstddef>

#include "remap_plan.h"

constexpr int FUSE_MAX_POINTS = LFVIO_FUSE_MAX_POINTS;
constexpr int FUSE_MIN_STEP = 12, FUSE_MAX_STEP = 1024;
constexpr int FUSE_THREADS = 256;  // all three kernels: one lane per point
constexpr int FUSE_KEPT = 0, FUSE_GATE = 1, FUSE_PROJECTION = 2;  // FuseHit::why, and the places of `counts`
constexpr unsigned FUSE_INF_BITS = 0x7f800000u;                   // what the range image is filled with

// ---- a point's bytes
struct FuseLayout {
  int step, ox, oy, oz, big;
  int dwords;  // step and the three offsets are multiples of 4: whole-dword loads (the cloud's first byte is 4-aligned)
};
inline FuseLayout fuse_layout(const LfvioFuseIn &in) {
  const int any = in.point_step | in.off_x | in.off_y | in.off_z;
  return FuseLayout{in.point_step, in.off_x, in.off_y, in.off_z, in.big_endian, (any & 3) == 0};
}
KB_HD float fuse_float(unsigned bits) {
  float v;
  __builtin_memcpy(&v, &bits, 4);
  return v;
}
KB_HD unsigned fuse_swap(unsigned w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }
// the four bytes at p, whatever p's alignment; big: the first byte is the most significant
KB_HD float fuse_field_bytes(const unsigned char *p, int big) {
  const unsigned b0 = p[0], b1 = p[1], b2 = p[2], b3 = p[3];
  return fuse_float(big ? (b0 << 24) | (b1 << 16) | (b2 << 8) | b3 : b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
}
// the dword at the 4-aligned p, as this (little-endian) machine loads it
KB_HD float fuse_field_dword(const unsigned char *p, int big) {
  unsigned w;
  __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
  return fuse_float(big ? fuse_swap(w) : w);
}
struct FuseXYZ { float x, y, z; };
KB_HD FuseXYZ fuse_read(const FuseLayout &l, const unsigned char *cloud, size_t k) {
  const unsigned char *p = cloud + k * (size_t)l.step;
  if (l.dwords) return {fuse_field_dword(p + l.ox, l.big), fuse_field_dword(p + l.oy, l.big), fuse_field_dword(p + l.oz, l.big)};
  return {fuse_field_bytes(p + l.ox, l.big), fuse_field_bytes(p + l.oy, l.big), fuse_field_bytes(p + l.oz, l.big)};
}

// ---- per point
struct FuseView {  // a kernel argument, by value
  double R[9], T[3], min_range, max_range;
  int kind, width, height;
  ProjCam cam;  // CAMERA; EQUIRECT: zero
};
inline FuseView fuse_view(const LfvioFuseIn &in, KbCache *kb = nullptr) {
  FuseView v = {};
  for (int k = 0; k < 9; k++) v.R[k] = in.R[k];
  for (int k = 0; k < 3; k++) v.T[k] = in.T[k];
  v.min_range = in.min_range, v.max_range = in.max_range;
  v.kind = in.kind, v.width = in.width, v.height = in.height;
  if (in.kind == LFVIO_FUSE_CAMERA) v.cam = proj_cam(*in.proj, kb);
  return v;
}

struct FuseHit {
  int index;    // row * width + col, or -1
  float range;  // (float)r; of a point the gate dropped too
  int why;      // FUSE_KEPT, FUSE_GATE, FUSE_PROJECTION
};

// the angle of atan2(X, Y) — the longitude, 0 along +Y, positive towards +X — for (X, Y) != (0, 0)
KB_HD double fuse_lon(double X, double Y) {
  constexpr double PI_HI = 3.14159265358979311600e+00, PI_LO = 1.22464679914735317723e-16, PIO2 = 1.57079632679489655800e+00;
  const double a = cam_atan(X / Y);
  if (Y > 0.0) return a;
  if (Y < 0.0) return X >= 0.0 ? PI_HI + (a + PI_LO) : (a - PI_LO) - PI_HI;
  return X > 0.0 ? PIO2 : X < 0.0 ? -PIO2 : a;  // Y == 0; (a NaN Y: a NaN)
}
struct FuseFrac { double fx, fy; };
// EQUIRECT's fractional pixel of a point off the pole: lon in [-pi, pi], lat in [-pi / 2, pi / 2], so 0 <= fx <= width, 0 <= fy <= height
KB_HD FuseFrac fuse_equirect(int width, int height, double X, double Y, double Z, double nxy) {
  constexpr double PI = 3.14159265358979323846;
  const double lon = fuse_lon(X, Y), lat = cam_atan(Z / nxy);
  return {(double)width * (0.5 + lon / (2.0 * PI)), (double)height * (0.5 - lat / PI)};
}

KB_HD FuseHit fuse_point(const FuseView &a, float x, float y, float z) {
  const double xd = (double)x, yd = (double)y, zd = (double)z;
  const double X = ((a.R[0] * xd + a.R[1] * yd) + a.R[2] * zd) + a.T[0];
  const double Y = ((a.R[3] * xd + a.R[4] * yd) + a.R[5] * zd) + a.T[1];
  const double Z = ((a.R[6] * xd + a.R[7] * yd) + a.R[8] * zd) + a.T[2];
  const double r = sqrt((X * X + Y * Y) + Z * Z);
  const float rf = (float)r;
  if (!(r > 0.0 && r >= a.min_range && r <= a.max_range && r < INFINITY)) return {-1, rf, FUSE_GATE};
  int col, row;
  if (a.kind == LFVIO_FUSE_EQUIRECT) {
    const double nxy = sqrt(X * X + Y * Y);
    if (nxy == 0.0) return {-1, rf, FUSE_PROJECTION};
    const FuseFrac f = fuse_equirect(a.width, a.height, X, Y, Z, nxy);
    col = (int)f.fx, row = (int)f.fy;  // both in [0, side]: finite, never negative
    if (col == a.width) col = 0;
    if (row == a.height) row = a.height - 1;
  } else {
    const CamPixel p = cam_project(a.cam, X, Y, Z);
    col = remap_index((float)p.u), row = remap_index((float)p.v);
    bool front = true;
    if (a.cam.t.model == LFVIO_CAM_PINHOLE) front = Z > 0.0;
    if (a.cam.t.model == LFVIO_CAM_MEI) front = Z + a.cam.t.xi * r > 0.0;
    if (!front) return {-1, rf, FUSE_PROJECTION};
  }
  if (!(col >= 0 && col < a.width && row >= 0 && row < a.height)) return {-1, rf, FUSE_PROJECTION};
  return {row * a.width + col, rf, FUSE_KEPT};  // at most 8192 * 8192 - 1: an int
}

// ---- the argument check: nullptr, or why the call is refused (what needs the context — REMAP's resident map — is fuse.inc's)
inline bool fuse_fields_overlap(int a, int b) { return a - b < 4 && b - a < 4; }
inline const char *fuse_check(const LfvioFuseIn *in, const LfvioFuseOut *out) {
  if (!in || !out) return "lfvio_cloud_fuse: null input or output";
  if (in->n < 0 || in->n > FUSE_MAX_POINTS) return "lfvio_cloud_fuse: n outside [0, 1 << 20]";
  if (in->n > 0 && !in->cloud) return "lfvio_cloud_fuse: null cloud";
  if (in->point_step < FUSE_MIN_STEP || in->point_step > FUSE_MAX_STEP) return "lfvio_cloud_fuse: point_step outside [12, 1024]";
  const int off[3] = {in->off_x, in->off_y, in->off_z};
  for (int o : off)
    if (o < 0 || o > in->point_step - 4) return "lfvio_cloud_fuse: a field offset outside [0, point_step - 4]";
  if (fuse_fields_overlap(off[0], off[1]) || fuse_fields_overlap(off[0], off[2]) || fuse_fields_overlap(off[1], off[2]))
    return "lfvio_cloud_fuse: two fields overlap";
  if (in->big_endian != 0 && in->big_endian != 1) return "lfvio_cloud_fuse: big_endian is neither 0 nor 1";
  for (double v : in->R)
    if (!std::isfinite(v)) return "lfvio_cloud_fuse: a non-finite R entry";
  for (double v : in->T)
    if (!std::isfinite(v)) return "lfvio_cloud_fuse: a non-finite T entry";
  if (!std::isfinite(in->min_range) || in->min_range < 0.0) return "lfvio_cloud_fuse: min_range negative or not finite";
  if (!(in->max_range >= in->min_range)) return "lfvio_cloud_fuse: max_range below min_range";
  if (in->kind != LFVIO_FUSE_EQUIRECT && in->kind != LFVIO_FUSE_CAMERA) return "lfvio_cloud_fuse: a kind other than LFVIO_FUSE_EQUIRECT and LFVIO_FUSE_CAMERA";
  if (remap_side_check(in->width, in->height)) return "lfvio_cloud_fuse: width or height outside [16, 8192]";
  if (in->kind == LFVIO_FUSE_CAMERA)
    if (const char *why = proj_check(in->proj)) return why;
  if (in->image_mode != LFVIO_FUSE_IMAGE_NONE && in->image_mode != LFVIO_FUSE_IMAGE_GIVEN && in->image_mode != LFVIO_FUSE_IMAGE_REMAP)
    return "lfvio_cloud_fuse: an unknown image_mode";
  if (in->image_mode == LFVIO_FUSE_IMAGE_NONE) {
    if (out->colour || out->image_out) return "lfvio_cloud_fuse: colour or image_out asked for without an image";
    return nullptr;
  }
  if (!in->pixels) return "lfvio_cloud_fuse: null pixels";
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  const bool given = in->image_mode == LFVIO_FUSE_IMAGE_GIVEN;
  return imgfmt_check(in->fmt ? *in->fmt : mono, given ? in->width : in->src_width, given ? in->height : in->src_height);
}

// ---- launch geometry: a lane per point
inline unsigned fuse_blocks(int n) { return (unsigned)((n + FUSE_THREADS - 1) / FUSE_THREADS); }
