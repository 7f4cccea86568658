// clahe_plan.h — the host-side plan of lfvio_clahe_set / lfvio_clahe_apply (include/lfvio.h): the argument checks, the extent of the
// tiled image, the tile size, the clip count and the three float factors the kernels take as arguments, so that every division happens
// once, on the host, in IEEE float.  Plain C++ (no HIP): clahe.inc uses it, tests/test_clahe_ref.py compiles it alone with g++ and
// holds it to tests/clahe_ref.py's plan().
#pragma once
#include "klt_plan.h"

constexpr double CLAHE_MAX_CLIP = 1024.0;
constexpr int CLAHE_BAND_ROWS = 16;  // rows of a tile one workgroup of k_clahe_hist counts; rows of the image one of k_clahe_map writes

struct ClahePlan {
  int ext_w, ext_h;  // the image continued right and down by reflect-101 (never materialised)
  int tw, th, area;  // of a tile
  int clip;          // bins are cut at this count; 0: no clipping
  float lut_scale, inv_tw, inv_th;
};

// nullptr, or what is wrong with the fields of *cfg
inline const char *clahe_check(const LfvioClaheIn *cfg) {
  if (!(cfg->clip_limit >= 0.0 && cfg->clip_limit <= CLAHE_MAX_CLIP)) return "lfvio_clahe: clip_limit outside [0, 1024]";
  if (cfg->tiles_x < 1 || cfg->tiles_x > LFVIO_CLAHE_MAX_TILES || cfg->tiles_y < 1 || cfg->tiles_y > LFVIO_CLAHE_MAX_TILES)
    return "lfvio_clahe: tiles_x or tiles_y outside [1, 16]";
  return nullptr;
}

inline const char *clahe_size_check(int width, int height) {
  if (width < KLT_MIN_SIDE || width > KLT_MAX_SIDE || height < KLT_MIN_SIDE || height > KLT_MAX_SIDE)
    return "lfvio_clahe_apply: width or height outside [16, 8192]";
  return nullptr;
}

// Both sides divide: the image's own size.  Otherwise each side grows by tiles - side % tiles: a whole `tiles` on a side that does
// divide, as OpenCV does it.  (area <= 8208^2 and clip <= 4 area fit an int.)
inline ClahePlan clahe_plan(int width, int height, const LfvioClaheIn &cfg) {
  ClahePlan p;
  const int tx = cfg.tiles_x, ty = cfg.tiles_y;
  const bool divides = width % tx == 0 && height % ty == 0;
  p.ext_w = divides ? width : width + (tx - width % tx);
  p.ext_h = divides ? height : height + (ty - height % ty);
  p.tw = p.ext_w / tx, p.th = p.ext_h / ty, p.area = p.tw * p.th;
  p.clip = 0;
  if (cfg.clip_limit != 0.0) {
    p.clip = (int)(cfg.clip_limit * (double)p.area / 256.0);
    if (p.clip < 1) p.clip = 1;
  }
  p.lut_scale = 255.0f / (float)p.area;
  p.inv_tw = 1.0f / (float)p.tw;
  p.inv_th = 1.0f / (float)p.th;
  return p;
}
