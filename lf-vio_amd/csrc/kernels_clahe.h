// kernels_clahe.h — CLAHE (cv::createCLAHE(clip, Size(tiles_x, tiles_y))->apply on 8 bits, feature_tracker.cpp:101-107) behind
// lfvio_clahe_apply and the equalize step of lfvio_klt_track; the algorithm is stated in include/lfvio.h and, as the specification,
// in tests/clahe_ref.py.  Three launches:
//
//   k_clahe_hist : grid (tiles, bands of CLAHE_BAND_ROWS rows of a tile).  A workgroup counts its band into a 256-bin LDS histogram
//                  with integer LDS atomics and adds its non-zero bins to the [tiles][256] int table with integer atomics: the sums do
//                  not depend on the order of arrival.  The tile lies in the image continued right and down by reflect-101; the
//                  continuation is index arithmetic, no extended image exists.
//   k_clahe_lut  : one workgroup of 256 per tile, one thread per bin: clip, redistribute, inclusive scan, scale, round half to even.
//                  It zeroes the table's row behind its read, so the table is ready for the next call.
//   k_clahe_map  : image-wide.  The rows of the image fall into tiles_y + 1 segments in which the two tile rows (ty1, ty2) of the
//                  blend are constant; a workgroup takes up to CLAHE_BAND_ROWS rows of one segment and 256 columns, keeps the LUTs of
//                  those two tile rows in LDS (at most 2 x 16 x 256 bytes), computes a column's tile indices and weights once per
//                  thread (4 columns each) and walks its rows.  Every float operation is rounded on its own (__fmul_rn, __fadd_rn,
//                  __fsub_rn: never contracted into a fused multiply-add, which gives other bytes).  VEC (width % 4 == 0): pixels are
//                  loaded and stored as uchar4.
#pragma once
#include "clahe_plan.h"
#include "kernels_klt.h"

constexpr int CLAHE_THREADS = 256;
constexpr int CLAHE_MAP_COLS = 256;  // columns of one workgroup of k_clahe_map: 64 threads of 4 pixels, 4 rows at a time

DEV void clahe_hist_body(const unsigned char *src, int W, int H, int tiles_x, int tw, int th, int *table) {
  __shared__ int bins[256];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int x0 = (tile % tiles_x) * tw, y0 = (tile / tiles_x) * th;
  const int r0 = blockIdx.y * CLAHE_BAND_ROWS, r1 = min(r0 + CLAHE_BAND_ROWS, th);
  bins[tid] = 0;
  __syncthreads();
  for (int r = r0 + (tid >> 6); r < r1; r += CLAHE_THREADS / 64) {
    const unsigned char *row = src + (size_t)klt_reflect(y0 + r, H) * W;
    for (int x = tid & 63; x < tw; x += 64) atomicAdd(&bins[row[klt_reflect(x0 + x, W)]], 1);
  }
  __syncthreads();
  const int n = bins[tid];
  if (n) atomicAdd(&table[tile * 256 + tid], n);
}
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_hist(const unsigned char *src, int W, int H, int tiles_x, int tw, int th, int *table) {
  clahe_hist_body(src, W, H, tiles_x, tw, th, table);
}

// inclusive sums of v over the 256 threads, through s[256]; every thread may read s[255] (the total) until the next barrier
DEV int clahe_scan(int v, int *s, int tid) {
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < 256; off <<= 1) {
    const int t = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}

DEV unsigned char clahe_u8(float v) { return (unsigned char)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

DEV void clahe_lut_body(int *table, int clip, float lut_scale, unsigned char *lut) {
  __shared__ int s[256];
  const int tid = threadIdx.x, at = blockIdx.x * 256 + tid;
  int h = table[at];
  table[at] = 0;
  if (clip > 0) {
    const int over = max(h - clip, 0);
    h = min(h, clip);
    clahe_scan(over, s, tid);
    const int clipped = s[255], batch = clipped / 256, rest = clipped - 256 * batch;
    __syncthreads();  // s is written again below
    h += batch;
    if (rest) {  // one more to the bins 0, step, 2 step, ...: rest * step <= 256, so all `rest` of them lie below 256
      const int step = max(256 / rest, 1);
      if (tid % step == 0 && tid / step < rest) h++;
    }
  }
  const int sum = clahe_scan(h, s, tid);
  lut[at] = clahe_u8(__fmul_rn((float)sum, lut_scale));
}
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_lut(int *table, int clip, float lut_scale, unsigned char *lut) {
  clahe_lut_body(table, clip, lut_scale, lut);
}

// floor(i * inv - 0.5): the (unclamped) first tile of pixel i of an axis
DEV float clahe_tf(int i, float inv) { return __fsub_rn(__fmul_rn((float)i, inv), 0.5f); }

// the first row in [0, H] whose unclamped first tile row is >= t (the formula is monotone in the row; the guess is off by one at most)
DEV int clahe_first_row(int t, int th, float inv_th, int H) {
  if (t < 0) return 0;
  int y = min(max(t * th + (th + 1) / 2, 0), H);
  while (y < H && (int)floorf(clahe_tf(y, inv_th)) < t) y++;
  while (y > 0 && (int)floorf(clahe_tf(y - 1, inv_th)) >= t) y--;
  return y;
}

template <bool VEC>
DEV void clahe_map_body(const unsigned char *src, unsigned char *dst, int W, int H, int tiles_x, int tiles_y, int th, int sub, float inv_tw, float inv_th,
                        const unsigned char *lut) {
  __shared__ __attribute__((aligned(16))) unsigned char L[2 * LFVIO_CLAHE_MAX_TILES * 256];
  const int tid = threadIdx.x;
  // segment s: the rows whose unclamped first tile row is s - 1; this workgroup's share of them
  const int s = blockIdx.y / sub, part = blockIdx.y - s * sub;
  const int lo = clahe_first_row(s - 1, th, inv_th, H), hi = s >= tiles_y ? H : clahe_first_row(s, th, inv_th, H);
  const int per = (hi - lo + sub - 1) / sub, y0 = lo + part * per, y1 = min(y0 + per, hi);
  if (y0 >= y1) return;  // (the whole workgroup)
  const int tyA = max(s - 1, 0), tyB = min(s, tiles_y - 1), row_bytes = tiles_x * 256;
  {
    const uint4 *a = (const uint4 *)(lut + (size_t)tyA * row_bytes), *b = (const uint4 *)(lut + (size_t)tyB * row_bytes);
    uint4 *la = (uint4 *)L, *lb = (uint4 *)(L + row_bytes);
    for (int i = tid; i < row_bytes / 16; i += CLAHE_THREADS) la[i] = a[i], lb[i] = b[i];
  }
  __syncthreads();
  const int x0 = blockIdx.x * CLAHE_MAP_COLS + (tid & 63) * 4;
  int o1[4], o2[4];  // offsets of the column's two tiles in a LUT row
  float xa[4], xa1[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float tf = clahe_tf(x0 + j, inv_tw), fl = floorf(tf);
    const int t = (int)fl;
    xa[j] = __fsub_rn(tf, fl), xa1[j] = __fsub_rn(1.0f, xa[j]);
    o1[j] = min(max(t, 0), tiles_x - 1) * 256, o2[j] = min(max(t + 1, 0), tiles_x - 1) * 256;
  }
  if (x0 >= W) return;  // (behind the only barrier)
  for (int y = y0 + (tid >> 6); y < y1; y += CLAHE_THREADS / 64) {
    const float tf = clahe_tf(y, inv_th), fl = floorf(tf);
    const int t = (int)fl;
    const float ya = __fsub_rn(tf, fl), ya1 = __fsub_rn(1.0f, ya);
    // the row's two tile rows are tyA or tyB: slot 0 or 1 of L
    const unsigned char *l1 = L + (min(max(t, 0), tiles_y - 1) == tyA ? 0 : row_bytes), *l2 = L + (min(max(t + 1, 0), tiles_y - 1) == tyA ? 0 : row_bytes);
    const size_t at = (size_t)y * W + x0;
    unsigned char v[4], o[4];
    if (VEC) {
      const uchar4 p = *(const uchar4 *)(src + at);
      v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = x0 + j < W ? src[at + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float a = (float)l1[o1[j] + v[j]], b = (float)l1[o2[j] + v[j]], c = (float)l2[o1[j] + v[j]], d = (float)l2[o2[j] + v[j]];
      const float top = __fadd_rn(__fmul_rn(a, xa1[j]), __fmul_rn(b, xa[j])), bottom = __fadd_rn(__fmul_rn(c, xa1[j]), __fmul_rn(d, xa[j]));
      o[j] = clahe_u8(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bottom, ya)));
    }
    if (VEC) {
      *(uchar4 *)(dst + at) = make_uchar4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (x0 + j < W) dst[at + j] = o[j];
    }
  }
}
template <bool VEC>
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_map(const unsigned char *src, unsigned char *dst, int W, int H, int tiles_x, int tiles_y, int th,
                                                             int sub, float inv_tw, float inv_th, const unsigned char *lut) {
  clahe_map_body<VEC>(src, dst, W, H, tiles_x, tiles_y, th, sub, inv_tw, inv_th, lut);
}
