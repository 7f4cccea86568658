// tracksource_plan.h — the host-side plan of lfvio_track_source_set (include/lfvio.h): the per-call check of a tracker
// call that takes its image through the resident map, the launch geometry of k_remap_gray (kernels_tracksource.h) and a host copy of
// one lane's arithmetic.  Plain C++ (no HIP): tracksource.inc uses it, tests/test_tracksource_plan.py compiles it alone with g++ and
// holds it to tests/tracksource_ref.py, tests/tools/tracksource_plan_walk.cpp walks it under the CPU sanitizers.
#pragma once
#include <cstddef>

#include "image_format.h"
#include "remap_plan.h"

// What lfvio_track_source_set stores: the SOURCE image's size (checked by remap_side_check at the set call)
struct TrackSourceState {
  bool on = false;
  int sw = 0, sh = 0;
};

// nullptr, or why a tracker call on a W x H image is refused while the setting is on: judged before anything is touched.  f: the
// image format setting (nullptr: off, which is mono8 with contiguous rows)
inline const char *tracksource_call_check(const TrackSourceState &s, const RemapResident &r, const LfvioImageFormat *f, int W, int H) {
  if (!s.on) return nullptr;
  if (!r.valid) return "lfvio_track_source: no resident map";
  if (r.width != W || r.height != H) return "lfvio_track_source: the resident map is of another size than width x height";
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  return imgfmt_check(f ? *f : mono, s.sw, s.sh);
}

// What such a call does: the source's geometry (the integer map's key), its encoding and the bytes that go up
struct TrackSourcePlan {
  RemapGeom g;
  int code;
  size_t bytes;
};
inline TrackSourcePlan tracksource_plan(const TrackSourceState &s, const LfvioImageFormat *f) {
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  const LfvioImageFormat &fm = f ? *f : mono;
  return TrackSourcePlan{remap_geom(fm, s.sw, s.sh), fm.encoding, imgfmt_bytes(fm, s.sw, s.sh)};
}

// ---- launch geometry: k_remap_apply's (one run of width * height pixels, a lane per REMAP_RUN of them)
inline unsigned tracksource_blocks(size_t pixels) { return remap_apply_blocks(pixels); }
inline size_t tracksource_lanes(size_t pixels) { return (size_t)tracksource_blocks(pixels) * REMAP_THREADS; }

// ---- one lane of k_remap_gray on the host, the kernel's arithmetic statement by statement: `lane` of tracksource_lanes(pixels).
// Reads imap[p] for p < pixels and src[o .. o + min(bpp, 3) - 1] for the entries o >= 0 (offset 0 for an outside one); writes
// level0[p] for the lane's own p < pixels.
inline void tracksource_lane(int code, const int *imap, const unsigned char *src, unsigned char *level0, size_t pixels, size_t lane) {
  const int bpp = imgfmt_bpp(code), nb = bpp < 3 ? bpp : 3;
  const size_t p0 = lane * REMAP_RUN;
  if (p0 >= pixels) return;
  const size_t p1 = p0 + REMAP_RUN <= pixels ? p0 + REMAP_RUN : pixels;
  for (size_t p = p0; p < p1; p++) {
    const int o = imap[p];
    const unsigned char *s = src + (o < 0 ? 0 : o);
    unsigned b[3] = {0u, 0u, 0u};
    for (int k = 0; k < nb; k++) b[k] = o < 0 ? 0u : (unsigned)s[k];
    level0[p] = (unsigned char)imgfmt_gray(code, b[0], b[1], b[2]);
  }
}
