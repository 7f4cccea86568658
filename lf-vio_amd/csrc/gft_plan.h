// gft_plan.h — the host-side plan of lfvio_gft_detect / lfvio_gft_set_mask (include/lfvio.h): the argument checks and the sizes of
// the candidate sort, its launches and the work arrays.  Plain C++ (no HIP): gft.inc, trackframe.inc and trackbatch.inc use it,
// tests/test_gft_ref.py compiles it alone with g++.
#pragma once
#include <cstddef>

#include "klt_plan.h"

constexpr int GFT_MAX_DIST = 1024;   // of min_distance and mask_radius
constexpr int GFT_CHUNK = 4096;      // candidates one workgroup orders in LDS (k_gft_sort_local)
constexpr int GFT_THREADS = 256;     // a workgroup of every kernel but k_gft_sort_local
constexpr int GFT_SORT_GRID = 512;   // workgroups of a launch of the sort network, at most
constexpr int GFT_LIST = LFVIO_GFT_MAX_CORNERS;  // of the kept points and of the accepted corners (= LFVIO_KLT_MAX_POINTS)

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

// The bitonic network over `capacity` entries, launch by launch: local(0) for the stages inside a chunk, then per stage
// k = 2 GFT_CHUNK .. capacity one global(k, j) per distance j = k / 2 .. GFT_CHUNK and one local(k) for the rest.  The single route
// launches k_gft_sort_local / _global from it, the batched route their _b variants.
template <class Local, class Global>
inline void gft_sort_stages(size_t capacity, Local local, Global global) {
  local(0u);
  for (size_t k = 2 * (size_t)GFT_CHUNK; k <= capacity; k *= 2) {
    for (size_t j = k / 2; j >= (size_t)GFT_CHUNK; j /= 2) global((unsigned)k, (unsigned)j);
    local((unsigned)k);
  }
}
inline int gft_sort_launches(size_t capacity) {
  int n = 0;
  gft_sort_stages(capacity, [&](unsigned) { n++; }, [&](unsigned, unsigned) { n++; });
  return n;
}
// ... and the grids of the two kernels: at most GFT_SORT_GRID workgroups each, which stride over the padded candidate count
struct GftSortGrid {
  unsigned chunks, halves;  // of k_gft_sort_local (a chunk per workgroup) and k_gft_sort_global (a pair per thread)
};
inline GftSortGrid gft_sort_grid(size_t capacity) {
  const size_t chunks = capacity / GFT_CHUNK, halves = capacity / 2 / GFT_THREADS;
  return GftSortGrid{(unsigned)(chunks < (size_t)GFT_SORT_GRID ? chunks : (size_t)GFT_SORT_GRID), (unsigned)(halves < (size_t)GFT_SORT_GRID ? halves : (size_t)GFT_SORT_GRID)};
}

// The detector's work arrays of one image size, one block: lambda, the candidates' keys and indices, the final mask, the kept
// pixels, GftDev.  GftOffsets is what a kernel of the batched route takes by value, beside the block's base.
struct GftDev {  // one call's state on the device
  unsigned long long max_bits;  // of the largest lambda under the final mask; 0: none
  int num_kept, num_cand;
};
struct GftOffsets {
  size_t lam, keys, idx, mask, kxy, st;
};
static_assert(sizeof(GftOffsets) == 48, "a kernel argument: six offsets");
struct GftWork : GftOffsets {
  size_t bytes, capacity;
};
inline GftWork gft_work(int W, int H) {
  GftWork o;
  const size_t px = (size_t)W * H;
  o.capacity = gft_capacity(W, H);
  size_t end = 0;
  auto take = [&](size_t bytes) {
    const size_t at = end;
    end = (end + bytes + 255) / 256 * 256;
    return at;
  };
  o.lam = take(px * 8), o.keys = take(o.capacity * 8), o.idx = take(o.capacity * 4), o.mask = take(px), o.kxy = take((size_t)GFT_LIST * 4);
  o.st = take(sizeof(GftDev)), o.bytes = end;
  return o;
}
