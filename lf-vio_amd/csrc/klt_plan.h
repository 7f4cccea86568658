// klt_plan.h — the host-side plan of lfvio_klt_track (include/lfvio.h): the argument check, the level sizes, levels_used and the
// offsets of the levels in a pyramid buffer.  Plain C++ (no HIP): klt.inc uses it, tests/test_klt_ref.py compiles it alone with g++
// and holds it to tests/klt_ref.py's plan().
#pragma once
#include <cstddef>

#include "../../include/lfvio.h"

constexpr int KLT_MIN_SIDE = 16, KLT_MAX_SIDE = 8192, KLT_MIN_WIN = 5, KLT_MAX_WIN = 41, KLT_MAX_ITER = 100;
constexpr int KLT_LEVELS = LFVIO_KLT_MAX_LEVEL + 1;
constexpr size_t KLT_ALIGN = 256;

struct KltPlan {
  int levels_used;        // the last level tracked
  int w[KLT_LEVELS], h[KLT_LEVELS];
  size_t off[KLT_LEVELS];  // of level k in a pyramid buffer; a function of the sizes of the levels below k alone
  size_t bytes;            // of levels 0 .. levels_used
};

// nullptr, or what is wrong with the fields of *in (the pointers for the outputs are the entry's to check)
inline const char *klt_check(const LfvioKltIn *in) {
  if (in->width < KLT_MIN_SIDE || in->width > KLT_MAX_SIDE || in->height < KLT_MIN_SIDE || in->height > KLT_MAX_SIDE)
    return "lfvio_klt_track: width or height outside [16, 8192]";
  if (!in->image) return "lfvio_klt_track: null image";
  if (in->num_points < 0 || in->num_points > LFVIO_KLT_MAX_POINTS) return "lfvio_klt_track: num_points outside [0, 4096]";
  if (in->num_points > 0 && !in->prev_pts) return "lfvio_klt_track: null prev_pts";
  if (in->win_size < KLT_MIN_WIN || in->win_size > KLT_MAX_WIN || in->win_size % 2 == 0) return "lfvio_klt_track: win_size not odd in [5, 41]";
  if (in->max_level < 0 || in->max_level > LFVIO_KLT_MAX_LEVEL) return "lfvio_klt_track: max_level outside [0, 5]";
  if (in->max_iterations < 1 || in->max_iterations > KLT_MAX_ITER) return "lfvio_klt_track: max_iterations outside [1, 100]";
  if (!(in->epsilon > 0.0)) return "lfvio_klt_track: epsilon not > 0";
  if (!(in->min_eig_threshold >= 0.0)) return "lfvio_klt_track: min_eig_threshold not >= 0";
  return nullptr;
}

// Level k + 1 is ((w_k + 1) / 2, (h_k + 1) / 2); building stops before the first level whose width or height is <= win and behind
// max_level.  (win = 0, max_level = LFVIO_KLT_MAX_LEVEL: every level a buffer of this image size can be asked to hold.)
inline KltPlan klt_plan(int width, int height, int win, int max_level) {
  KltPlan p = {};
  p.w[0] = width, p.h[0] = height;
  int L = 0;
  while (L < max_level) {
    const int nw = (p.w[L] + 1) / 2, nh = (p.h[L] + 1) / 2;
    if (nw <= win || nh <= win) break;
    L++;
    p.w[L] = nw, p.h[L] = nh;
  }
  p.levels_used = L;
  size_t end = 0;
  for (int k = 0; k <= L; k++) {
    p.off[k] = end;
    end = (end + (size_t)p.w[k] * (size_t)p.h[k] + KLT_ALIGN - 1) / KLT_ALIGN * KLT_ALIGN;
  }
  p.bytes = end;
  return p;
}
