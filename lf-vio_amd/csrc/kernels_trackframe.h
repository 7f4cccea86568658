// kernels_trackframe.h — what lfvio_track_frame (include/lfvio.h, trackframe.inc) adds between the stages of the separate calls, so
// that no count has to come down to the host: reduceVector, the sample sets, the merge of setMask's order with the new corners and
// the numbering of updateID.  The stages themselves are the kernels of kernels_klt.h, kernels_clahe.h, kernels_gft.h,
// kernels_twoview.h and kernels_track.h; those that took a count as an argument have a variant (k_*_n) that reads it from TfDev.
//
// Each kernel is ONE workgroup of TF_THREADS over at most LFVIO_TRACK_MAX_POINTS entries.  Thread t owns the TF_PER consecutive
// entries from t * TF_PER: it counts its keepers, an exclusive scan over the workgroup's counts (tf_scan) gives its first output
// slot, and it writes its keepers in order — the output keeps the input's order, as reduceVector does.
//
//   k_tf_flow   : entries with status != 0 of (cur, next, ids, cnt) -> (cur1, forw1, ids1, cnt1 + 1); n1.  Then, strided over the S
//                 sample sets, trackframe_draw (trackframe_plan.h) over n1 where n1 >= 8.  Writes every count of TfDev, so that a
//                 call without the later stages (publish == 0) leaves them defined.
//   k_tf_reject : entries with mask != 0 of (forw1, ids1, cnt1) -> (forw2, ids2, cnt2); n2.  (cur is not needed behind rejectWithF.)
//   k_tf_finish : the next table.  With detection: [forw2[kept[i]] for i < num_kept | corners], the corners with id -1 and count 1;
//                 without: (forw1, ids1, cnt1) as they are.  ids_raw keeps the -1 for k_trk_undist_n; in the table every -1 takes
//                 n_id + (the number of -1 before it).  Written twice: into the context's other table buffer and into the block that
//                 goes down to the host.  num_points, num_new.
//   k_tf_message: lfvio_track_frame_message only, behind k_trk_undist_n.  Entries with track_cnt > 1 of the table that goes down and of
//                 undistortedPoints' outputs -> the nine-float rows of the node's feature message (feature_tracker_node.cpp:113-170), in
//                 table order; num_rows.  The ids are the numbered ones k_tf_finish wrote, not ids_raw.  Count and scan as the others;
//                 the scan leaves every entry's row in LDS and the write goes over (row, column) with the whole workgroup.
#pragma once
#include "kernels_gft.h"
#include "kernels_track.h"
#include "trackframe_plan.h"

constexpr int TF_THREADS = 256, TF_PER = LFVIO_TRACK_MAX_POINTS / TF_THREADS;
static_assert(TF_PER * TF_THREADS == LFVIO_TRACK_MAX_POINTS && LFVIO_TRACK_MAX_POINTS == LFVIO_KLT_MAX_POINTS, "one thread, TF_PER entries");

// a table as three arrays: [n][2] floats, ids, counts.  (TfDev, the counts every kernel here reads and writes: trackframe_plan.h)
struct TfTable {
  float *pts;
  int *ids, *cnt;
};
// [n][2] floats | n ids | n counts at p
__host__ __device__ inline TfTable tf_table(char *p, size_t n) { return TfTable{(float *)p, (int *)(p + n * 8), (int *)(p + n * 12)}; }

// Exclusive scan of v over the workgroup (Hillis-Steele on two rows of LDS); total: the sum, in every thread.
DEV int tf_scan(int v, int (*s)[TF_THREADS], int &total) {
  const int tid = threadIdx.x;
  int row = 0;
  s[0][tid] = v;
  __syncthreads();
  for (int d = 1; d < TF_THREADS; d <<= 1) {
    s[1 - row][tid] = s[row][tid] + (tid >= d ? s[row][tid - d] : 0);
    row = 1 - row;
    __syncthreads();
  }
  const int incl = s[row][tid];
  total = s[row][TF_THREADS - 1];
  __syncthreads();  // (s may be used again)
  return incl - v;
}

// (the bodies are device functions: kernels_trackbatch.h runs the same code per slot)
DEV void tf_flow_body(int n0, const unsigned char *status, const float *cur, const float *next, const int *ids, const int *cnt, float *cur1,
                      const TfTable &t1, TfDev *dev, int S, const unsigned *words, int *samples) {
  __shared__ int s[2][TF_THREADS];
  const int tid = threadIdx.x, first = tid * TF_PER, last = min(first + TF_PER, n0);
  int mine = 0;
  for (int i = first; i < last; i++) mine += status[i] != 0;
  int n1;
  int at = tf_scan(mine, s, n1);
  for (int i = first; i < last; i++)
    if (status[i] != 0) {
      cur1[2 * at] = cur[2 * i], cur1[2 * at + 1] = cur[2 * i + 1];
      t1.pts[2 * at] = next[2 * i], t1.pts[2 * at + 1] = next[2 * i + 1];
      t1.ids[at] = ids[i], t1.cnt[at] = cnt[i] + 1;
      at++;
    }
  if (tid == 0) dev->n1 = n1, dev->n2 = n1, dev->num_points = n1, dev->num_new = 0;
  if (words && n1 >= TRACK_MIN_MATCHES)
    for (int k = tid; k < S; k += TF_THREADS) {
      unsigned w[8];
      int out[8];
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = words[8 * k + j];
      trackframe_draw(w, n1, out);
#pragma unroll
      for (int j = 0; j < 8; j++) samples[8 * k + j] = out[j];
    }
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_flow(int n0, const unsigned char *status, const float *cur, const float *next, const int *ids,
                                                        const int *cnt, float *cur1, TfTable t1, TfDev *dev, int S, const unsigned *words,
                                                        int *samples) {
  tf_flow_body(n0, status, cur, next, ids, cnt, cur1, t1, dev, S, words, samples);
}

DEV void tf_reject_body(const unsigned char *mask, const TfTable &t1, const TfTable &t2, TfDev *dev) {
  __shared__ int s[2][TF_THREADS];
  const int n1 = dev->n1, tid = threadIdx.x, first = tid * TF_PER, last = min(first + TF_PER, n1);
  int mine = 0;
  for (int i = first; i < last; i++) mine += mask[i] != 0;
  int n2;
  int at = tf_scan(mine, s, n2);
  for (int i = first; i < last; i++)
    if (mask[i] != 0) {
      t2.pts[2 * at] = t1.pts[2 * i], t2.pts[2 * at + 1] = t1.pts[2 * i + 1];
      t2.ids[at] = t1.ids[i], t2.cnt[at] = t1.cnt[i];
      at++;
    }
  if (tid == 0) dev->n2 = n2;
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_reject(const unsigned char *mask, TfTable t1, TfTable t2, TfDev *dev) {
  tf_reject_body(mask, t1, t2, dev);
}

// src: (forw2, ids2, cnt2) with detect (kept, corners, dev->detect), otherwise (forw1, ids1, cnt1) and kept, corners unused
DEV void tf_finish_body(int detect, const TfTable &src, const int *kept, const float *corners, int n_id, const TfTable &next, const TfTable &down,
                        int *ids_raw, TfDev *dev) {
  __shared__ int s[2][TF_THREADS];
  const int nk = detect ? dev->detect.num_kept : dev->n1, n = nk + (detect ? dev->detect.num_corners : 0);
  const int tid = threadIdx.x, first = tid * TF_PER, last = min(first + TF_PER, n);
  int id[TF_PER];
  int mine = 0;
#pragma unroll
  for (int e = 0; e < TF_PER; e++) {
    const int i = first + e;
    int v = 0;
    if (i < last) {
      float x, y;
      int c;
      if (i < nk) {
        const int j = detect ? kept[i] : i;
        x = src.pts[2 * j], y = src.pts[2 * j + 1], v = src.ids[j], c = src.cnt[j];
      } else {
        x = corners[2 * (i - nk)], y = corners[2 * (i - nk) + 1], v = -1, c = 1;
      }
      next.pts[2 * i] = x, next.pts[2 * i + 1] = y, next.cnt[i] = c;
      down.pts[2 * i] = x, down.pts[2 * i + 1] = y, down.cnt[i] = c;
      ids_raw[i] = v;
      mine += v == -1;
    }
    id[e] = v;
  }
  int num_new;
  int at = n_id + tf_scan(mine, s, num_new);
#pragma unroll
  for (int e = 0; e < TF_PER; e++) {
    const int i = first + e;
    if (i < last) {
      const int v = id[e] == -1 ? at++ : id[e];
      next.ids[i] = v, down.ids[i] = v;
    }
  }
  if (tid == 0) dev->num_points = n, dev->num_new = num_new;
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_finish(int detect, TfTable src, const int *kept, const float *corners, int n_id, TfTable next,
                                                          TfTable down, int *ids_raw, TfDev *dev) {
  tf_finish_body(detect, src, kept, corners, n_id, next, down, ids_raw, dev);
}

// rows: [cap][9] = un_pts_3d | (float)(id * NUM_OF_CAM + 0), NUM_OF_CAM = 1 | pts | velocity_3d; cap: the host's bound on num_points
DEV void tf_message_body(const TfDev *dev, int cap, const TfTable &down, const float *un_pts_3d, const float *velocity_3d, int *num_rows, float *rows) {
  __shared__ int s[2][TF_THREADS];
  __shared__ int slot[LFVIO_TRACK_MAX_POINTS];  // the row of entry i, or -1
  const int n = min(dev->num_points, cap), tid = threadIdx.x, first = tid * TF_PER, last = min(first + TF_PER, n);
  int c[TF_PER];
  int mine = 0;
#pragma unroll
  for (int e = 0; e < TF_PER; e++) {
    c[e] = first + e < last ? down.cnt[first + e] : 0;
    mine += c[e] > 1;
  }
  int total;
  int at = tf_scan(mine, s, total);
#pragma unroll
  for (int e = 0; e < TF_PER; e++)
    if (first + e < last) slot[first + e] = c[e] > 1 ? at++ : -1;
  __syncthreads();
  // the ordered write, an element a thread: the rows are short (150 entries in the node's configuration), sixteen of them one after
  // the other in a thread would be sixteen round trips to memory
  for (int k = tid; k < 9 * n; k += TF_THREADS) {
    const int i = k / 9, col = k - 9 * i, o = slot[i];
    if (o < 0) continue;
    float v;
    if (col < 3)
      v = un_pts_3d[3 * i + col];
    else if (col == 3)
      v = (float)down.ids[i];  // (int -> float: nearest even)
    else if (col < 6)
      v = down.pts[2 * i + col - 4];
    else
      v = velocity_3d[3 * i + col - 6];
    rows[9 * o + col] = v;
  }
  if (tid == 0) *num_rows = total;
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_message(const TfDev *dev, int cap, TfTable down, const float *un_pts_3d, const float *velocity_3d,
                                                           int *num_rows, float *rows) {
  tf_message_body(dev, cap, down, un_pts_3d, velocity_3d, num_rows, rows);
}
