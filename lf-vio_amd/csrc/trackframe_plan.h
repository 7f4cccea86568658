// trackframe_plan.h — the host side of lfvio_track_frame (include/lfvio.h) that needs no device: the argument check, which calls
// the checks of the separate calls (klt_check, gft_check, track_common_check) on the fields the frame shares with them, and the
// bounds the host knows for the counts that stay on the device, and everything behind the copy down — the counts against their
// bounds, then the caller's arrays from a down segment — which lfvio_track_batch_frame does per slot with the same functions.  Plain
// C++ (no HIP): trackframe.inc and trackbatch.inc use it, tests/test_track_frame_ref.py compiles it alone with g++ and holds it to the
// checks of tests/track_frame_ref.py, tests/tools/track_batch_plan_walk.cpp walks the download under the CPU sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gft_plan.h"
#include "track_plan.h"

// the flow's and the detection's inputs as the separate calls take them, without points
inline LfvioKltIn trackframe_klt(const LfvioTrackFrameIn *in) {
  LfvioKltIn k = {};
  k.width = in->width, k.height = in->height, k.image = in->image;
  k.win_size = in->win_size, k.max_level = in->max_level, k.max_iterations = in->max_iterations;
  k.epsilon = in->epsilon, k.min_eig_threshold = in->min_eig_threshold, k.border = in->border;
  return k;
}
inline LfvioGftIn trackframe_gft(const LfvioTrackFrameIn *in) {
  LfvioGftIn g = {};
  g.max_count = in->max_count, g.quality_level = in->quality_level, g.min_distance = in->min_distance, g.mask_radius = in->mask_radius;
  return g;
}

// nullptr, or what is wrong with the fields of *in beside a table of table_count entries (the pointers of out are the entry's to check)
inline const char *trackframe_check(const LfvioTrackFrameIn *in, int table_count) {
  const LfvioKltIn k = trackframe_klt(in);
  if (const char *why = klt_check(&k)) return why;
  const LfvioGftIn g = trackframe_gft(in);
  if (const char *why = gft_check(&g)) return why;
  if (const char *why = track_common_check(in->camera, 0)) return why;
  if (in->num_samples < 1 || in->num_samples > TRACK_MAX_SAMPLES) return "lfvio_track_frame: num_samples outside [1, 1024]";
  if (in->publish && !in->sample_words) return "lfvio_track_frame: null sample_words";
  if (in->capacity < std::max(in->max_count, table_count) || in->capacity > LFVIO_TRACK_MAX_POINTS)
    return "lfvio_track_frame: capacity below max(max_count, the table's count) or above 4096";
  if (std::isnan(in->time)) return "lfvio_track_frame: time is NaN";
  return nullptr;
}

// lfvio_track_frame_message's own: the message it fills.  (rows has in->capacity rows, and a message has at most as many as the table.)
inline const char *trackframe_message_check(const LfvioTrackMessage *msg) {
  if (!msg || !msg->rows) return "lfvio_track_frame_message: null msg or msg->rows";
  return nullptr;
}
// bytes of the message's segment of the block that comes down: [num_rows | pad to 16 | bound x 9 floats]
constexpr size_t TF_MSG_HEAD = 16;
inline size_t trackframe_message_bytes(size_t bound) { return TF_MSG_HEAD + bound * 36; }

// What the host knows of the counts: n1 and n2 are at most the table's count, the count after the call at most this.
inline int trackframe_bound(int table_count, int max_count, bool publish) { return publish ? std::max(table_count, max_count) : table_count; }

// ---- behind the copy down, for lfvio_track_frame and for every slot of lfvio_track_batch_frame alike
struct TfDev {  // one call's counts and records on the device; the head of the segment that comes down
  int n1, n2, num_points, num_new;
  LfvioTrackRejectOut reject;  // k_trk_fit_n
  LfvioGftOut detect;          // k_gft_pick
};
static_assert(sizeof(TfDev) == 136, "the kernels of both routes and the staging layouts share it");

// every array of out, and of the message where one is given, is there
inline bool trackframe_out_check(const LfvioTrackFrameOut *out, const LfvioTrackMessage *msg) {
  return out->pts && out->ids && out->track_cnt && out->un_pts && out->un_pts_3d && out->velocity_3d && (!msg || msg->rows);
}

// Every count the device wrote lies within the bound the host sized its segment and the caller's arrays by: nothing below is
// copied by a count that fails here.  num_rows: the head of the message's segment (0 where none came down).
inline bool trackframe_counts_check(const TfDev &v, int table_count, int max_count, bool publish, int num_rows) {
  if (v.num_points < 0 || v.num_points > trackframe_bound(table_count, max_count, publish)) return false;
  if (v.n1 < 0 || v.n1 > table_count || num_rows < 0 || num_rows > v.num_points) return false;
  return !publish || (v.detect.num_kept >= 0 && v.detect.num_kept <= table_count && v.detect.num_corners >= 0 && v.detect.num_corners <= max_count);
}

// the scalars of an LfvioTrackFrameOut, everything in front of its arrays
inline void trackframe_zero(LfvioTrackFrameOut *o) {
  o->num_points = o->num_new = o->levels_used = o->num_tracked = o->num_after_reject = 0;
  std::memset(&o->reject, 0, sizeof o->reject);
  std::memset(&o->detect, 0, sizeof o->detect);
}

struct TfDown {  // one down segment on the host
  const TfDev *dev;
  const char *table;  // [B][2] floats | B ids | B counts
  size_t B;
  const char *un, *un3d, *vel;  // undistortedPoints' outputs, B entries each
  const char *msg;              // [num_rows | pad to TF_MSG_HEAD | B rows], or null: no rows came down
};
// *out, and *msg where given, from a segment whose counts passed trackframe_counts_check: the scalars (no model: E is zero), the
// first num_points entries of every array, the first num_rows rows
inline void trackframe_emit(const TfDown &d, int levels_used, bool publish, LfvioTrackFrameOut *out, LfvioTrackMessage *msg) {
  const TfDev &v = *d.dev;
  const size_t n = (size_t)v.num_points;
  trackframe_zero(out);
  out->num_points = v.num_points, out->num_new = v.num_new, out->levels_used = levels_used, out->num_tracked = v.n1, out->num_after_reject = v.n2;
  if (publish) {
    track_reject_copy(&out->reject, v.reject);
    out->detect = v.detect;
  }
  std::memcpy(out->pts, d.table, n * 8);
  std::memcpy(out->ids, d.table + d.B * 8, n * 4);
  std::memcpy(out->track_cnt, d.table + d.B * 12, n * 4);
  std::memcpy(out->un_pts, d.un, n * 8);
  std::memcpy(out->un_pts_3d, d.un3d, n * 12);
  std::memcpy(out->velocity_3d, d.vel, n * 12);
  if (msg) {
    msg->num_rows = d.msg ? *(const int *)d.msg : 0;
    if (msg->num_rows) std::memcpy(msg->rows, d.msg + TF_MSG_HEAD, (size_t)msg->num_rows * 36);
  }
}

// Sample set from eight words over n >= 8 matches (include/lfvio.h, step 3): the k-th draw is the (words[k] % (n - k))-th of the
// indices not yet chosen.  The same function on the device (kernels_trackframe.h) and on the host.
#if defined(__HIPCC__)
#define TF_HD __host__ __device__ inline
#define TF_UNROLL _Pragma("unroll")
#else
#define TF_HD inline
#define TF_UNROLL
#endif
// (Fixed trip counts and constant indices once unrolled: on the device `chosen` stays in registers.)
TF_HD void trackframe_draw(const unsigned *words, int n, int *out) {
  int chosen[8] = {};  // the first k entries: the indices drawn so far, ascending
  TF_UNROLL
  for (int k = 0; k < 8; k++) {
    int r = (int)(words[k] % (unsigned)(n - k));
    TF_UNROLL
    for (int j = 0; j < 8; j++)
      if (j < k && r >= chosen[j]) r++;  // (ascending: once r is below one of them it is below the rest)
    out[k] = r;
    chosen[k] = r;
    TF_UNROLL
    for (int j = 7; j > 0; j--)
      if (j <= k && chosen[j - 1] > chosen[j]) {
        const int t = chosen[j];
        chosen[j] = chosen[j - 1], chosen[j - 1] = t;
      }
  }
}
