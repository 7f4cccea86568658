// trackbatch_source_plan.h — the host side of lfvio_track_batch_map / lfvio_track_batch_source (include/lfvio.h) that
// needs no device: what a slot's resident remap is, the per-call check of a batch frame that takes its images through the slots'
// maps, the decision when the integer maps are rebuilt and a host copy of one lane of k_remap_gray_b (kernels_trackbatch.h).  The
// per-slot layout of the maps and its alignment are trackbatch_plan.h's (TbMaps).  Plain C++ (no HIP): trackbatch.inc uses it,
// tests/test_trackbatch_source_plan.py compiles it alone with g++ and tests/tools/track_batch_source_walk.cpp walks it under the CPU
// sanitizers.
#pragma once
#include "trackbatch_plan.h"
#include "tracksource_plan.h"

// What a slot holds of its map between calls: the float maps of a width x height output are a finished build's
struct TbMapInfo {
  bool valid = false;
  int width = 0, height = 0;
};

// lfvio_track_batch_source's own check: remap_side_check, as lfvio_track_source_set's
inline const char *trackbatch_source_set_check(int src_width, int src_height) { return remap_side_check(src_width, src_height); }

// nullptr, or why a batch frame is refused while the setting is on: judged before anything is touched.  in[0 .. count): the call's
// entries, already through trackbatch_frame_check (the active ones agree on width x height); maps[i]: slot i's; f: the batch's
// format setting (nullptr: off, which is mono8 with contiguous rows).  The order is the single route's (tracksource_call_check): the
// maps before the format.  Idle slots need no map.
inline const char *trackbatch_source_check(const TrackSourceState &s, const LfvioImageFormat *f, int count, const LfvioTrackFrameIn *in, const TbMapInfo *maps) {
  if (!s.on) return nullptr;
  for (int i = 0; i < count; i++) {
    if (!trackbatch_active(in[i])) continue;
    if (!maps[i].valid) return "lfvio_track_batch_frame: an active slot has no map (lfvio_track_batch_map)";
    if (maps[i].width != in[i].width || maps[i].height != in[i].height) return "lfvio_track_batch_frame: an active slot's map is of another size than width x height";
  }
  const LfvioImageFormat mono = {LFVIO_IMG_MONO8, 0};
  return imgfmt_check(f ? *f : mono, s.sw, s.sh);
}

// ---- whose the integer maps are.  The source geometry is the batch's, so ONE record says what every mapped slot's integer map was
// written for: a frame call of another geometry rebuilds all of them in one launch (k_remap_index_b) and a steady stream never does;
// a map built later is written for the record's geometry at the build (trackbatch_build_geom), so the record stays true of every slot.
struct TbIndexed {
  bool indexed = false;
  RemapGeom geom = {0, 0, 0, 0};
};
inline bool trackbatch_needs_index(const TbIndexed &r, const RemapGeom &now) {
  RemapResident one;
  one.valid = true, one.indexed = r.indexed, one.geom = r.geom;
  return remap_needs_index(one, now);
}
// the geometry a build writes its integer map for (bpp 0: none yet — the first frame writes them all)
inline RemapGeom trackbatch_build_geom(const TbIndexed &r) { return r.indexed ? r.geom : RemapGeom{0, 0, 0, 0}; }

// ---- one lane of k_remap_gray_b on the host: tracksource_lane on slot `slot`'s integer map, found in the maps' block as the kernel
// finds it.  Reads pixels ints at maps + slot * stride + index_at and the source as tracksource_lane does; writes level0[p] for the
// lane's own p < pixels.
inline const int *trackbatch_slot_index(const char *maps, const TbMaps &lay, int slot) { return (const int *)(maps + (size_t)slot * lay.stride() + lay.index_at()); }
inline void trackbatch_source_lane(int code, const char *maps, const TbMaps &lay, int slot, const unsigned char *src, unsigned char *level0, size_t pixels, size_t lane) {
  tracksource_lane(code, trackbatch_slot_index(maps, lay, slot), src, level0, pixels, lane);
}
