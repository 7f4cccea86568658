// gft_plan.h — the host-side plan of lfvio_gft_detect / lfvio_gft_set_mask (include/lfvio.h): the argument checks and the sizes of
// the candidate sort.  Plain C++ (no HIP): gft.inc uses it, tests/test_gft_ref.py compiles it alone with g++.
#pragma once
#include <cstddef>

#include "klt_plan.h"

constexpr int GFT_MAX_DIST = 1024;   // of min_distance and mask_radius
constexpr int GFT_CHUNK = 4096;      // candidates one workgroup orders in LDS (k_gft_sort_local)

// nullptr, or what is wrong with the fields of *in (the pointers for the outputs are the entry's to check)
inline const char *gft_check(const LfvioGftIn *in) {
  if (in->num_points < 0 || in->num_points > LFVIO_KLT_MAX_POINTS) return "lfvio_gft_detect: num_points outside [0, 4096]";
  if (in->num_points > 0 && (!in->pts || !in->track_cnt)) return "lfvio_gft_detect: null pts or track_cnt";
  if (in->max_count < 1 || in->max_count > LFVIO_GFT_MAX_CORNERS) return "lfvio_gft_detect: max_count outside [1, 4096]";
  if (!(in->quality_level > 0.0 && in->quality_level <= 1.0)) return "lfvio_gft_detect: quality_level outside (0, 1]";
  if (in->min_distance < 0 || in->min_distance > GFT_MAX_DIST) return "lfvio_gft_detect: min_distance outside [0, 1024]";
  if (in->mask_radius < 0 || in->mask_radius > GFT_MAX_DIST) return "lfvio_gft_detect: mask_radius outside [0, 1024]";
  return nullptr;
}

// a base mask of width x height beside a resident image of image_w x image_h (image_w = 0: none resident)
inline const char *gft_mask_check(int width, int height, int image_w, int image_h) {
  if (width < KLT_MIN_SIDE || width > KLT_MAX_SIDE || height < KLT_MIN_SIDE || height > KLT_MAX_SIDE)
    return "lfvio_gft_set_mask: width or height outside [16, 8192]";
  if (image_w && (width != image_w || height != image_h)) return "lfvio_gft_set_mask: not the resident image's size";
  return nullptr;
}

// The candidate arrays hold a power of two of entries, at least one chunk and at least every pixel of the image: a plateau makes
// every interior pixel a candidate.
inline size_t gft_capacity(int width, int height) {
  size_t p = GFT_CHUNK;
  while (p < (size_t)width * (size_t)height) p *= 2;
  return p;
}

// launches of the bitonic network over `capacity` entries: one k_gft_sort_local for the stages inside a chunk, then per stage
// k = 2 GFT_CHUNK .. capacity one k_gft_sort_global per distance j = k / 2 .. GFT_CHUNK and one k_gft_sort_local for the rest
inline int gft_sort_launches(size_t capacity) {
  int n = 1;
  for (size_t k = 2 * (size_t)GFT_CHUNK; k <= capacity; k *= 2) {
    for (size_t j = k / 2; j >= (size_t)GFT_CHUNK; j /= 2) n++;
    n++;
  }
  return n;
}
