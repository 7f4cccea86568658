// remap_plan.h — the host-side plan of lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply (include/lfvio.h): the
// argument checks, the ray and the map entry of one output pixel, the index of a map entry (remap_index: cv::saturate_cast<short>), the
// integer map's entry, the decision when that map is rebuilt and the launch geometry.  Plain C++ (no HIP); the per-pixel functions
// are host-and-device functions under hipcc (KB_HD of camera_kb.h), so k_remap_build (kernels_remap.h) and the host run the same
// text.  remap.inc uses it, tests/test_remap_plan.py compiles it alone with g++ and holds it to tests/project_ref.py,
// tests/tools/remap_plan_walk.cpp walks it under the CPU sanitizers.
//
// remap_index is WRITTEN DOWN FROM MEMORY of OpenCV 3.3's RemapInvoker / remapNearest (the float maps go through
// saturate_cast<short>, which is cvRound — round to nearest, ties to even — and a clamp to [-32768, 32767]; BORDER_CONSTANT writes the
// border value where the index is outside the source): no OpenCV was at hand and nobody has compared them, as for image_format.h.
#pragma once
#include <cmath>
#include <cstddef>

#include "camera_models.h"
#include "image_format.h"

constexpr int REMAP_MAX_POINTS = 1 << 20;
constexpr int REMAP_TILE_W = 32, REMAP_TILE_H = 8;    // k_remap_build: one workgroup's tile of output pixels, a lane each
constexpr int REMAP_THREADS = REMAP_TILE_W * REMAP_TILE_H;
constexpr int REMAP_RUN = 4;                          // k_remap_apply: consecutive output pixels of one lane
constexpr int REMAP_PROJECT_THREADS = 64;             // k_cam_project: one lane per point

// ---- the source image an integer map was written for
struct RemapGeom {
  int sw, sh, step, bpp;  // step in bytes, never 0 here (imgfmt_step); bpp 0: none
};
inline bool operator==(const RemapGeom &a, const RemapGeom &b) { return a.sw == b.sw && a.sh == b.sh && a.step == b.step && a.bpp == b.bpp; }
inline RemapGeom remap_geom(const LfvioImageFormat &f, int sw, int sh) { return RemapGeom{sw, sh, (int)imgfmt_step(f, sw), imgfmt_bpp(f.encoding)}; }

// What a context holds between calls: the float maps of a width x height output, and the integer map of the last source geometry
struct RemapResident {
  bool valid = false;       // the float maps are a finished build's
  int width = 0, height = 0;
  bool indexed = false;     // the integer map is theirs, for `geom`
  RemapGeom geom = {0, 0, 0, 0};
};
// k_remap_apply reads the integer map alone: it is rebuilt from the float maps whenever the source's width, height, step or bytes
// per pixel differ from what it was written for (a build writes it for the geometry of the last apply, so a steady stream never does)
inline bool remap_needs_index(const RemapResident &r, const RemapGeom &now) { return !r.indexed || !(r.geom == now); }

// ---- per map entry
// cv::saturate_cast<short>(float): round to nearest, ties to even, clamped.  A NaN gives -32768: outside every image.  Nothing that can
// be NaN, infinite or huge is converted to an integer.
KB_HD int remap_index(float v) {
  float r = rintf(v);
  r = r >= -32768.0f ? r : -32768.0f;
  r = r > 32767.0f ? 32767.0f : r;
  return (int)r;
}
// the source pixel's byte offset, or -1 (at most 8191 * 65536 + 8191 * 4: an int)
KB_HD int remap_offset(float mx, float my, const RemapGeom &g) {
  const int sx = remap_index(mx), sy = remap_index(my);
  return (sx >= 0 && sx < g.sw && sy >= 0 && sy < g.sh) ? sy * g.step + sx * g.bpp : -1;
}

// the ray of output pixel (i, j).  EQUIRECT: GetremapMat (pointcloud_image_fusion.cpp:93-101), sine and cosine by kb_sincos — held to 50
// digits on [-pi, pi] as it is (tests/test_project_ref.py), so no symmetry is applied.  PERSPECTIVE: M (i, j, 1), row-major
KB_HD CamRay remap_ray(int kind, int width, int height, const double *M, int i, int j) {
  constexpr double PI = 3.14159265358979323846;
  if (kind == LFVIO_MAP_PERSPECTIVE) {
    const double u = (double)i, v = (double)j;
    return {(M[0] * u + M[1] * v) + M[2], (M[3] * u + M[4] * v) + M[5], (M[6] * u + M[7] * v) + M[8]};
  }
  const double lon = ((double)i / (double)width - 0.5) * (2.0 * PI);
  const double lat = -(((double)j / (double)height - 0.5) * PI);
  double slon, clon, slat, clat;
  kb_sincos(lon, slon, clon);
  kb_sincos(lat, slat, clat);
  return {clat * slon, clat * clon, slat};
}
struct RemapEntry { float x, y; };
KB_HD RemapEntry remap_entry(const ProjCam &cam, int kind, int width, int height, const double *M, int i, int j) {
  const CamRay P = remap_ray(kind, width, height, M, i, j);
  const CamPixel p = cam_project(cam, P.x, P.y, P.z);
  return {(float)p.u, (float)p.v};
}

// ---- the argument checks: nullptr, or why the call is refused
inline const char *remap_side_check(int width, int height) {
  if (width < IMGFMT_MIN_SIDE || width > IMGFMT_MAX_SIDE || height < IMGFMT_MIN_SIDE || height > IMGFMT_MAX_SIDE)
    return "lfvio_remap: width or height outside [16, 8192]";
  return nullptr;
}
inline const char *remap_project_check(const LfvioProjector *proj, int n, const double *P, const double *px) {
  if (const char *why = proj_check(proj)) return why;
  if (n < 0 || n > REMAP_MAX_POINTS) return "lfvio_cam_project: n outside [0, 1 << 20]";
  if (n > 0 && (!P || !px)) return "lfvio_cam_project: null P or px";
  return nullptr;
}
inline const char *remap_build_check(const LfvioRemapIn *in, const float *map_x, const float *map_y) {
  if (!in) return "lfvio_remap_build: null input";
  if (const char *why = proj_check(in->proj)) return why;
  if (in->kind != LFVIO_MAP_EQUIRECT && in->kind != LFVIO_MAP_PERSPECTIVE) return "lfvio_remap_build: a kind other than LFVIO_MAP_EQUIRECT and LFVIO_MAP_PERSPECTIVE";
  if (in->kind == LFVIO_MAP_PERSPECTIVE)
    for (double x : in->M)
      if (!std::isfinite(x)) return "lfvio_remap_build: a non-finite M entry";
  if (const char *why = remap_side_check(in->width, in->height)) return why;
  if (!map_x != !map_y) return "lfvio_remap_build: exactly one of map_x and map_y is null";
  return nullptr;
}
// fmt nullptr: mono8, rows contiguous (as lfvio_image_gray)
inline const char *remap_apply_check(const LfvioImageFormat *fmt, int src_width, int src_height, const unsigned char *pixels, const unsigned char *out) {
  if (!pixels || !out) return "lfvio_remap_apply: null pixels or out";
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  return imgfmt_check(fmt ? *fmt : mono, src_width, src_height);
}

// ---- launch geometry
struct RemapGrid { unsigned x, y; };
inline RemapGrid remap_build_grid(int width, int height) {
  return RemapGrid{(unsigned)((width + REMAP_TILE_W - 1) / REMAP_TILE_W), (unsigned)((height + REMAP_TILE_H - 1) / REMAP_TILE_H)};
}
// k_remap_apply: output and maps are contiguous, so the image is ONE run of width * height pixels; a lane takes REMAP_RUN of them (its
// stores are whole dwords at 4-aligned offsets whatever the row's byte length), the last lane the tail of fewer, byte by byte
inline unsigned remap_apply_blocks(size_t pixels) {
  const size_t lanes = (pixels + REMAP_RUN - 1) / REMAP_RUN;
  return (unsigned)((lanes + REMAP_THREADS - 1) / REMAP_THREADS);
}
inline unsigned remap_project_blocks(int n) { return (unsigned)((n + REMAP_PROJECT_THREADS - 1) / REMAP_PROJECT_THREADS); }
