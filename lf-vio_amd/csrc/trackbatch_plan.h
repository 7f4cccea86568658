// trackbatch_plan.h — the host side of the lfvio_track_batch_* calls (include/lfvio.h) that needs no device: the argument check of
// every batch call (trackframe_check per active entry, then the agreement rule), the bounds the host sizes grids and segments by,
// the slot's descriptor as the kernels read it, the layout of the staging block as plain functions that return offsets, the bytes
// one slot owns at a given image size, and the layout of a slot's resident remap (TbMaps; trackbatch_source_plan.h uses it).
// Plain C++ (no HIP): trackbatch.inc uses it, tests/test_track_batch_ref.py compiles it alone with g++ and
// tests/tools/track_batch_plan_walk.cpp walks it under the CPU sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <initializer_list>

#include "track_stream.h"
#include "trackframe_plan.h"

constexpr size_t TB_ALIGN = 256;
inline size_t tb_align(size_t v) { return (v + TB_ALIGN - 1) / TB_ALIGN * TB_ALIGN; }

// ---- the checks
inline const char *trackbatch_reserve_check(int slots) {
  if (slots < 0 || slots > LFVIO_TRACK_BATCH_MAX_SLOTS) return "lfvio_track_batch_reserve: slots outside [0, 64]";
  return nullptr;
}
// slot of lfvio_track_batch_set_mask / _reset: -1 (every slot) or an index below the reserved count
inline const char *trackbatch_slot_check(int slot, int slots) {
  if (slots < 1) return "lfvio_track_batch: no slots reserved";
  if (slot < -1 || slot >= slots) return "lfvio_track_batch: slot outside [-1, slots)";
  return nullptr;
}

// lfvio_track_batch_level: one slot (never -1), a resident image in it, a level that some call has built
inline const char *trackbatch_level_check(int slot, int slots, bool resident, int level, int built) {
  if (slot < 0 || slot >= slots) return "lfvio_track_batch_level: slot outside [0, slots)";
  if (!resident || level < 0 || level > built) return "lfvio_track_batch_level: no resident image, or a level that is not built";
  return nullptr;
}

inline bool trackbatch_active(const LfvioTrackFrameIn &in) { return in.image != nullptr; }

// the fourteen fields the active entries of one call share
inline const char *trackbatch_agree(const LfvioTrackFrameIn &a, const LfvioTrackFrameIn &b) {
  if (a.width != b.width || a.height != b.height) return "lfvio_track_batch_frame: active entries of different width or height";
  if (a.win_size != b.win_size || a.max_level != b.max_level || a.max_iterations != b.max_iterations || a.epsilon != b.epsilon ||
      a.min_eig_threshold != b.min_eig_threshold || a.border != b.border)
    return "lfvio_track_batch_frame: active entries of different flow settings";
  if (a.max_count != b.max_count || a.quality_level != b.quality_level || a.min_distance != b.min_distance || a.mask_radius != b.mask_radius)
    return "lfvio_track_batch_frame: active entries of different detection settings";
  if (a.num_samples != b.num_samples || a.capacity != b.capacity) return "lfvio_track_batch_frame: active entries of different num_samples or capacity";
  return nullptr;
}

// nullptr, or what is wrong with in[0 .. count) beside `slots` reserved slots whose tables hold table_counts[i] entries (the pointers
// of out and msg and the masks are the entry's to check)
inline const char *trackbatch_frame_check(int slots, int count, const LfvioTrackFrameIn *in, const int *table_counts) {
  if (slots < 1) return "lfvio_track_batch_frame: no slots reserved";
  if (count != slots) return "lfvio_track_batch_frame: count is not the reserved slot count";
  int first = -1;
  for (int i = 0; i < count; i++) {
    if (!trackbatch_active(in[i])) continue;
    if (const char *why = trackframe_check(&in[i], table_counts[i])) return why;
    if (first < 0) first = i;
    else if (const char *why = trackbatch_agree(in[first], in[i])) return why;
  }
  return nullptr;
}

// ---- the bounds
struct TbBounds {
  int active, publishing, first;  // counts of active / active and publishing entries; the first active entry (-1: none)
  int n0_max, B_max;              // the largest table count and the largest trackframe_bound among the active slots
};
inline TbBounds trackbatch_bounds(int count, const LfvioTrackFrameIn *in, const int *table_counts) {
  TbBounds b = {0, 0, -1, 0, 0};
  for (int i = 0; i < count; i++) {
    if (!trackbatch_active(in[i])) continue;
    if (b.first < 0) b.first = i;
    b.active++, b.publishing += in[i].publish != 0;
    b.n0_max = std::max(b.n0_max, table_counts[i]);
    b.B_max = std::max(b.B_max, trackframe_bound(table_counts[i], in[i].max_count, in[i].publish != 0));
  }
  return b;
}

// ---- the slot as the kernels read it: one entry per slot of the device array at the head of the staging block.  Uniform over a
// workgroup (blockIdx.z picks it); an entry with active == 0 holds nothing else but map_px.  It holds numbers only: WHERE a slot's
// memory lies follows from the slot's index and TbMem, a kernel argument, so that every pointer a kernel forms starts at a pointer
// argument.
struct TbSlot {
  int active, publish;
  int n0;          // entries of the resident table
  int n_id;        // the next id
  int prev_count;  // pairs in the previous map
  int prev_built;  // levels the pyramid tracked from holds above level 0 (the fresh one: all of this call's)
  int same;        // a pyramid of this image size is resident: track from it.  0: the fresh one is both images
  int pcur, tcur, mcur;  // which of the two pyramid buffers, tables and maps is the resident one; the call writes the other
  int masked;      // a base mask is set
  int image_k, words_k;  // the slot's image among the active slots' and its words among the publishing slots' in the staging block
  int map_px;      // pixels of the slot's resident remap (lfvio_track_batch_map), 0: none.  Filled for idle slots too (k_remap_index_b)
  double dt;       // time - the previous call's
  TrackCam cam;
};
// what a slot's stream (track_stream.h) says to a call on a W x H image that uses LU levels, at time `time`
inline void trackbatch_describe(TbSlot &t, const TrackStream &s, int W, int H, int LU, double time) {
  t.n0 = s.count, t.n_id = s.n_id, t.prev_count = s.mcount;
  t.prev_built = s.prev_built(W, H, LU), t.same = s.resident(W, H);
  t.pcur = s.pcur, t.tcur = s.tcur, t.mcur = s.mcur, t.masked = s.mask_set;
  t.dt = time - s.time;
}
struct TbMem {  // the bases and strides of the slots' memory
  char *stage, *fixed, *image, *clahe;  // the staging block; per slot: tables and maps | [pyramid | pyramid | mask | work] | CLAHE table and LUTs
  size_t image_stride, pyr, mask_at, work_at, clahe_stride;
  size_t words_at, words_stride, images_at, images_stride;  // in the staging block
  char *maps;                                                // per slot: [map_x | map_y | integer map] (TbMaps below); nullptr: no slot has a map
  size_t maps_stride, maps_y_at, maps_index_at;
};

// ---- the staging block: [descriptors | words of the publishing slots | images of the active slots] goes up; every slot has a segment
// for what lives between the stages and one for what comes down, the latter back to back so that one copy brings all of them.
struct TbShape {
  int slots, publishing, active;
  size_t n0_max, B_max, S, max_count, pixels, dev_bytes;  // dev_bytes: sizeof(TfDev)
  bool rows;                                               // the message's segment
};
struct TbStage {
  size_t desc, words, images, in_end;
  size_t mid, mid_stride, down, down_stride, end;
  // inside a slot's mid segment
  size_t c1, t1, t2, bl, br, A, score, E, raw, matched, next, status, samples, mask, kept, corners;
  // inside a slot's down segment
  size_t dev, table, un, un3d, vel, msg;
};
inline TbStage trackbatch_stage(const TbShape &s) {
  TbStage o = {};
  size_t end = 0;
  auto take = [&](size_t bytes) {
    const size_t at = tb_align(end);
    end = at + bytes;
    return at;
  };
  o.desc = take((size_t)s.slots * sizeof(TbSlot));
  o.words = take((size_t)s.publishing * tb_align(s.S * 32));
  o.images = take((size_t)s.active * tb_align(s.pixels));
  o.in_end = end;
  const size_t top = end;
  end = 0;
  const size_t N0 = s.n0_max, B = s.B_max;
  o.c1 = take(N0 * 8), o.t1 = take(N0 * 16), o.t2 = take(N0 * 16), o.bl = take(N0 * 24), o.br = take(N0 * 24);
  o.A = take(std::max<size_t>(N0, 9) * 72), o.score = take(s.S * 4), o.E = take(s.S * 72), o.raw = take(B * 4), o.matched = take(B * 4);
  o.next = take(N0 * 8), o.status = take(N0), o.samples = take(s.S * 32), o.mask = take(N0), o.kept = take(N0 * 4), o.corners = take(s.max_count * 8);
  o.mid_stride = tb_align(end);
  end = 0;
  o.dev = take(s.dev_bytes), o.table = take(B * 16), o.un = take(B * 8), o.un3d = take(B * 12), o.vel = take(B * 12);
  o.msg = s.rows ? take(trackframe_message_bytes(B)) : 0;
  o.down_stride = tb_align(end);
  o.mid = tb_align(top);
  o.down = o.mid + (size_t)s.slots * o.mid_stride;
  o.end = o.down + (size_t)s.slots * o.down_stride;
  return o;
}
// the k-th publishing slot's words, the k-th active slot's image, slot i's segments
inline size_t trackbatch_words_at(const TbStage &o, const TbShape &s, int k) { return o.words + (size_t)k * tb_align(s.S * 32); }
inline size_t trackbatch_image_at(const TbStage &o, const TbShape &s, int k) { return o.images + (size_t)k * tb_align(s.pixels); }
inline size_t trackbatch_mid_at(const TbStage &o, int slot) { return o.mid + (size_t)slot * o.mid_stride; }
inline size_t trackbatch_down_at(const TbStage &o, int slot) { return o.down + (size_t)slot * o.down_stride; }

// ---- the slot's memory.  Whatever the image size: two track tables and two (id, un_pts_3d) maps.  At an image size: two pyramid
// buffers, the base mask and the detector's arrays, [pyramid | pyramid | mask | work] — the segments keep their capacity when a
// smaller image follows, and grow to the largest seen.
constexpr size_t TB_FIXED_BYTES = 2 * TRACK_TABLE_BYTES + 2 * TRACK_MAP_BYTES;
constexpr size_t trackbatch_table_at(int which) { return (size_t)which * TRACK_TABLE_BYTES; }
constexpr size_t trackbatch_map_at(int which) { return 2 * TRACK_TABLE_BYTES + (size_t)which * TRACK_MAP_BYTES; }

struct TbImage {
  size_t pyr, mask, work;  // capacities, aligned
  size_t stride() const { return 2 * pyr + mask + work; }
  size_t pyr_at(int which) const { return (size_t)which * pyr; }
  size_t mask_at() const { return 2 * pyr; }
  size_t work_at() const { return 2 * pyr + mask; }
};
// work_bytes: of the detector's arrays at this size (0: a mask alone is being set)
inline TbImage trackbatch_image(int width, int height, size_t work_bytes) {
  TbImage m;
  m.pyr = tb_align(klt_plan(width, height, 0, LFVIO_KLT_MAX_LEVEL).bytes);
  m.mask = tb_align((size_t)width * (size_t)height);
  m.work = tb_align(work_bytes);
  return m;
}
inline bool trackbatch_image_covers(const TbImage &have, const TbImage &need) {
  return have.pyr >= need.pyr && have.mask >= need.mask && have.work >= need.work;
}
inline TbImage trackbatch_image_grown(const TbImage &have, const TbImage &need) {
  return TbImage{std::max(have.pyr, need.pyr), std::max(have.mask, need.mask), std::max(have.work, need.work)};
}
inline size_t trackbatch_slot_bytes(int width, int height, size_t work_bytes) { return TB_FIXED_BYTES + trackbatch_image(width, height, work_bytes).stride(); }

// ---- the slot's resident remap (lfvio_track_batch_map): the two float maps and the integer map of a width x height OUTPUT image, 12
// bytes per output pixel, [map_x | map_y | integer map] with every plane's capacity `px` pixels — the largest output any slot's map
// was built for; the planes keep their capacity when a smaller map follows.
// ALIGNMENT, stated here and checked by trackbatch_maps_aligned / trackbatch_level0_aligned: k_remap_gray_b loads the integer map
// sixteen bytes at a time and stores level 0 a dword at a time.  Every plane is tb_align'ed and so is the stride, and the block is an
// allocation of its own (256-aligned), so every slot's integer map starts 256-aligned; level 0 of either pyramid buffer starts at
// slot * TbImage::stride() + which * pyr, multiples of TB_ALIGN as well.  The source image is read by bytes: its place in the staging
// block and its step need no alignment.
struct TbMaps {
  size_t px;  // capacity of a plane, in pixels
  size_t plane() const { return tb_align(px * 4); }
  size_t x_at() const { return 0; }
  size_t y_at() const { return plane(); }
  size_t index_at() const { return 2 * plane(); }
  size_t stride() const { return 3 * plane(); }
};
inline TbMaps trackbatch_maps(int width, int height) { return TbMaps{(size_t)width * (size_t)height}; }
inline bool trackbatch_maps_covers(const TbMaps &have, const TbMaps &need) { return have.px >= need.px; }
inline TbMaps trackbatch_maps_grown(const TbMaps &have, const TbMaps &need) { return TbMaps{std::max(have.px, need.px)}; }
// every slot's integer map 256-aligned behind a 256-aligned base, the float maps with it
inline bool trackbatch_maps_aligned(const TbMaps &m, int slots) {
  for (int i = 0; i < slots; i++)
    for (size_t at : {m.x_at(), m.y_at(), m.index_at()})
      if (((size_t)i * m.stride() + at) % TB_ALIGN) return false;
  return true;
}
// level 0 of either pyramid buffer of every slot 4-aligned behind a 256-aligned base
inline bool trackbatch_level0_aligned(const TbImage &lay, int slots) {
  for (int i = 0; i < slots; i++)
    for (int which = 0; which < 2; which++)
      if (((size_t)i * lay.stride() + lay.pyr_at(which)) % 4) return false;
  return true;
}
