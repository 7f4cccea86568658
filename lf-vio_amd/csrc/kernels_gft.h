// kernels_gft.h — setMask and cv::goodFeaturesToTrack (feature_tracker.cpp:46-83, :147-176) behind lfvio_gft_detect; the algorithm
// is stated in include/lfvio.h and, as the specification, in tests/gft_ref.py.  Everything up to S and D is integer arithmetic,
// lambda is three correctly rounded double operations, every order below is total: the outputs are the specification's bits and do
// not depend on the order in which workgroups run.
//
//   k_gft_thin        : one workgroup.  Ranks the tracked points by (count descending, index ascending) by counting, then walks them
//                       in that order (gft_greedy): kept indices, kept pixels, their number.  Resets the call's GftDev.  A template
//                       over how the count arrives: an int (lfvio_gft_detect) or a pointer to it on the device (lfvio_track_frame).
//   k_gft_response    : 32 x 8 tiles.  The image with a halo of 2 (reflect-101) in LDS, the three Sobel products with a halo of 1 —
//                       a product outside the image is the product AT the reflected pixel, not the product of the reflected image's
//                       gradients — their 3 x 3 sums, S, D, lambda as double.  The final mask per tile: the base-mask byte and the
//                       kept points whose disc reaches the tile.  The masked maximum: per workgroup, then one atomicMax on the bit
//                       pattern of the non-negative double.
//   k_gft_cand        : 256 x 8 pixels per workgroup, a column per thread; candidates are appended as (lambda bits, pixel index): counted
//                       in LDS, one atomicAdd per workgroup on the global count (one per wave measured 145 us at 1280 x 960: ~15 000
//                       returning atomics on one address).  The append order is arbitrary, the pairs are unique.
//   k_gft_sort_local  : a bitonic network over launches orders the pairs descending (larger lambda, then larger index, first):
//   k_gft_sort_global   steps at distances below GFT_CHUNK run in LDS, one chunk per workgroup; longer ones in global memory.  The
//                       host enqueues the network of the arrays' capacity with grids of at most GFT_SORT_GRID workgroups, which
//                       stride over the padded candidate count; a launch of a stage beyond it returns at once.
//   k_gft_pick        : one workgroup walks the ordered candidates (gft_greedy) until the budget is reached; writes LfvioGftOut.
#pragma once
#include "dev_math.h"
#include "gft_plan.h"
#include "kernels_klt.h"

constexpr int GFT_TX = 32, GFT_TY = 8;  // (GFT_THREADS, GFT_SORT_GRID, GFT_LIST and GftDev: gft_plan.h)
constexpr int GFT_RAW_W = GFT_TX + 4, GFT_RAW_H = GFT_TY + 4, GFT_PRD_W = GFT_TX + 2, GFT_PRD_H = GFT_TY + 2;
constexpr int GFT_SORT_THREADS = 512;
constexpr int GFT_CAND_ROWS = 8;  // rows of 256 pixels per workgroup of k_gft_cand
static_assert(LFVIO_GFT_MAX_CORNERS == LFVIO_KLT_MAX_POINTS, "one list length for both greedy passes");
static_assert(GFT_TX * GFT_TY == GFT_THREADS, "a pixel per thread");

// a pixel as one int: y << 16 | x (both < 8192); negative: no pixel
DEV int gft_pack(int x, int y) { return y << 16 | x; }
DEV int gft_dist2(int p, int q) {
  const int dx = (p & 0xffff) - (q & 0xffff), dy = (p >> 16) - (q >> 16);
  return dx * dx + dy * dy;
}

// One workgroup of GFT_THREADS walks the items 0 .. n - 1 in order.  Item p has the pixel xy(p) (negative: never accepted) and is
// accepted when no accepted pixel lies at a squared distance < lim; the walk ends at `cap` accepted.  In batches of the workgroup's
// width: every thread tests its item against the accepted list, then the batch is resolved in order — a barrier per accepted item.
// The count is held by every thread alike, so every branch is workgroup-uniform.  acc: the accepted pixels (LDS, cap entries);
// batch: GFT_THREADS ints of LDS; emit(slot, p, pixel) is called by thread 0.  Returns the number accepted.
template <class XY, class Emit>
DEV int gft_greedy(int n, int lim, int cap, XY xy, Emit emit, int *acc, int *batch) {
  const int tid = threadIdx.x;
  int have = 0;
  for (int b = 0; b < n && have < cap; b += GFT_THREADS) {
    const int p = b + tid;
    int q = p < n ? xy(p) : -1;
    for (int a = 0; q >= 0 && a < have; a++)
      if (gft_dist2(q, acc[a]) < lim) q = -1;
    batch[tid] = q;
    __syncthreads();
    const int m = min(GFT_THREADS, n - b);
    for (int i = 0; i < m && have < cap; i++) {
      const int v = batch[i];  // (written before the last barrier: the same value in every thread)
      if (v < 0) continue;
      if (tid == 0) acc[have] = v, emit(have, b + i, v);
      if (tid > i && q >= 0 && gft_dist2(q, v) < lim) q = -1, batch[tid] = -1;
      have++;
      __syncthreads();
    }
    __syncthreads();  // (everybody is done with batch[] and sees acc[])
  }
  return have;
}

// a count as a kernel argument, or read from the device where the host knows only a bound of it (lfvio_track_frame)
DEV int gft_count(int n) { return n; }
DEV int gft_count(const int *n) { return *n; }

// Count = int: lfvio_gft_detect's N.  Count = const int *: N from the device; N = 0 runs no loop below and writes num_kept = 0.
// (the bodies are device functions: kernels_trackbatch.h runs the same code per slot)
DEV void gft_thin_body(int N, const float *pts, const int *cnt, const unsigned char *base, int W, int H, int r, GftDev *st, int *kept, int *kxy) {
  __shared__ int s_cnt[GFT_LIST];  // the counts, then the kept pixels
  __shared__ int s_xy[GFT_LIST], s_idx[GFT_LIST];  // pixel and index of the point of rank k
  __shared__ int s_batch[GFT_THREADS];
  const int tid = threadIdx.x;
  for (int i = tid; i < N; i += GFT_THREADS) s_cnt[i] = cnt[i];
  __syncthreads();
  for (int i = tid; i < N; i += GFT_THREADS) {
    const int ci = s_cnt[i];
    int rank = 0;
    for (int j = 0; j < N; j++) {
      const int cj = s_cnt[j];
      rank += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
    }
    const double rx = rint((double)pts[2 * i]), ry = rint((double)pts[2 * i + 1]);  // half to even, like cvRound; NaN fails the test
    int q = -1;
    if (rx >= 0.0 && rx < (double)W && ry >= 0.0 && ry < (double)H) {
      const int px = (int)rx, py = (int)ry;
      if (!base || base[(size_t)py * W + px] == 255) q = gft_pack(px, py);
    }
    s_xy[rank] = q, s_idx[rank] = i;
  }
  __syncthreads();
  const int nk = gft_greedy(
      N, r * r + 1, GFT_LIST, [&](int p) { return s_xy[p]; }, [&](int slot, int p, int v) { kept[slot] = s_idx[p], kxy[slot] = v; }, s_cnt, s_batch);
  if (tid == 0) st->max_bits = 0ull, st->num_kept = nk, st->num_cand = 0;
}
template <class Count>
__global__ __launch_bounds__(GFT_THREADS) void k_gft_thin(Count n_arg, const float *pts, const int *cnt, const unsigned char *base, int W, int H, int r,
                                                           GftDev *st, int *kept, int *kxy) {
  gft_thin_body(gft_count(n_arg), pts, cnt, base, W, H, r, st, kept, kxy);
}

DEV void gft_response_body(const unsigned char *img, int W, int H, const unsigned char *base, const int *kxy, int r, int max_count, GftDev *st,
                           double *lam, unsigned char *mask) {
  __shared__ unsigned char raw[GFT_RAW_H][GFT_RAW_W];
  __shared__ int pxx[GFT_PRD_H][GFT_PRD_W], pxy[GFT_PRD_H][GFT_PRD_W], pyy[GFT_PRD_H][GFT_PRD_W];
  __shared__ int s_disc[GFT_LIST], s_nd;
  __shared__ unsigned long long s_red[GFT_THREADS];
  const int nk = st->num_kept;
  if (max_count - nk <= 0) return;  // no budget: nothing is detected
  const int tid = threadIdx.x, x0 = blockIdx.x * GFT_TX, y0 = blockIdx.y * GFT_TY;
  if (tid == 0) s_nd = 0;
  for (int k = tid; k < GFT_RAW_H * GFT_RAW_W; k += GFT_THREADS) {  // raw[j][i] = pixel (x0 - 2 + i, y0 - 2 + j)
    const int j = k / GFT_RAW_W, i = k - j * GFT_RAW_W;
    raw[j][i] = img[(size_t)klt_reflect(y0 - 2 + j, H) * W + klt_reflect(x0 - 2 + i, W)];
  }
  __syncthreads();
  const int x1 = min(x0 + GFT_TX, W) - 1, y1 = min(y0 + GFT_TY, H) - 1, r2 = r * r;
  for (int k = tid; k < nk; k += GFT_THREADS) {  // the kept points whose disc reaches the tile (in any order: they are only OR-ed)
    const int q = kxy[k], qx = q & 0xffff, qy = q >> 16;
    if (gft_dist2(q, gft_pack(min(max(qx, x0), x1), min(max(qy, y0), y1))) <= r2) s_disc[atomicAdd(&s_nd, 1)] = q;
  }
  for (int k = tid; k < GFT_PRD_H * GFT_PRD_W; k += GFT_THREADS) {  // products at pixel (x0 - 1 + i, y0 - 1 + j), reflected INTO the image
    const int j = k / GFT_PRD_W, i = k - j * GFT_PRD_W;
    // (a position further outside than one pixel belongs to no output of the image: the clamp only keeps its reads inside raw)
    const int li = min(max(klt_reflect(x0 - 1 + i, W) - (x0 - 2), 1), GFT_RAW_W - 2), lj = min(max(klt_reflect(y0 - 1 + j, H) - (y0 - 2), 1), GFT_RAW_H - 2);
    const int a00 = raw[lj - 1][li - 1], a01 = raw[lj - 1][li], a02 = raw[lj - 1][li + 1], a10 = raw[lj][li - 1], a12 = raw[lj][li + 1];
    const int a20 = raw[lj + 1][li - 1], a21 = raw[lj + 1][li], a22 = raw[lj + 1][li + 1];
    const int dx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20), dy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
    pxx[j][i] = dx * dx, pxy[j][i] = dx * dy, pyy[j][i] = dy * dy;
  }
  __syncthreads();
  const int tx = tid % GFT_TX, ty = tid / GFT_TX, x = x0 + tx, y = y0 + ty;
  unsigned long long bits = 0ull;
  if (x < W && y < H) {
    int a = 0, b = 0, c = 0;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) a += pxx[ty + j][tx + i], b += pxy[ty + j][tx + i], c += pyy[ty + j][tx + i];
    const long long S = (long long)a + c, dac = (long long)a - c, D = dac * dac + 4ll * b * b;  // D <= 4.4e14 < 2^53: exact as double
    const double l = 0.5 * ((double)S - sqrt((double)D));
    const size_t p = (size_t)y * W + x;
    lam[p] = l;
    bool open = !base || base[p] != 0;
    const int me = gft_pack(x, y), nd = s_nd;
    for (int k = 0; open && k < nd; k++) open = gft_dist2(me, s_disc[k]) > r2;
    mask[p] = open ? 255 : 0;
    if (open) bits = (unsigned long long)__double_as_longlong(l);  // lambda >= 0: the bit patterns order like the values
  }
  s_red[tid] = bits;
  __syncthreads();
  for (int s = GFT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] = max(s_red[tid], s_red[tid + s]);
    __syncthreads();
  }
  // (the value only grows: a workgroup that sees one at least as large already has nothing to add)
  if (tid == 0 && s_red[0] > *(volatile unsigned long long *)&st->max_bits) atomicMax(&st->max_bits, s_red[0]);
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_response(const unsigned char *img, int W, int H, const unsigned char *base, const int *kxy, int r,
                                                               int max_count, GftDev *st, double *lam, unsigned char *mask) {
  gft_response_body(img, W, H, base, kxy, r, max_count, st, lam, mask);
}

DEV void gft_cand_body(const double *lam, const unsigned char *mask, int W, int H, double quality, int max_count, GftDev *st, unsigned long long *ck,
                       unsigned *ci) {
  __shared__ int s_count, s_first;
  if (max_count - st->num_kept <= 0 || st->max_bits == 0ull) return;
  const double thr = quality * __longlong_as_double((long long)st->max_bits);
  const int x = blockIdx.x * GFT_THREADS + threadIdx.x, y0 = blockIdx.y * GFT_CAND_ROWS;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  unsigned found = 0;  // bit k: (x, y0 + k) is a candidate
  if (x >= 1 && x <= W - 2) {
    for (int k = 0; k < GFT_CAND_ROWS; k++) {
      const int y = y0 + k;
      if (y < 1 || y > H - 2) continue;
      const size_t p = (size_t)y * W + x;
      const double l = lam[p];
      if (l > thr && mask[p]) {
        const double *u = lam + p - W, *d = lam + p + W;
        if (l >= u[-1] && l >= u[0] && l >= u[1] && l >= lam[p - 1] && l >= lam[p + 1] && l >= d[-1] && l >= d[0] && l >= d[1]) found |= 1u << k;  // the UNMASKED map
      }
    }
  }
  int at = found ? atomicAdd(&s_count, __popc(found)) : 0;  // (in LDS; any order)
  __syncthreads();
  if (threadIdx.x == 0 && s_count) s_first = atomicAdd(&st->num_cand, s_count);
  __syncthreads();
  at += s_first;
  for (int k = 0; k < GFT_CAND_ROWS; k++)
    if (found >> k & 1u) {
      const size_t p = (size_t)(y0 + k) * W + x;
      ck[at] = (unsigned long long)__double_as_longlong(lam[p]), ci[at] = (unsigned)p, at++;
    }
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_cand(const double *lam, const unsigned char *mask, int W, int H, double quality, int max_count, GftDev *st,
                                                           unsigned long long *ck, unsigned *ci) {
  gft_cand_body(lam, mask, W, H, quality, max_count, st, ck, ci);
}

// the padded length of the network: a power of two, at least one chunk
DEV unsigned gft_padded(int n) {
  unsigned p = GFT_CHUNK;
  while (p < (unsigned)n) p <<= 1;
  return p;
}
DEV bool gft_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) { return ka > kb || (ka == kb && ia > ib); }
// pair t of a step at distance j: the lower index (a zero bit put into t at j's position)
DEV unsigned gft_lower(unsigned t, unsigned j) { return ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); }

// stage = 0: loads a chunk (entries behind the candidates are (0, 0): behind every candidate, whose lambda is > 0), runs the stages
// k = 2 .. GFT_CHUNK on it.  Otherwise: the steps j = GFT_CHUNK / 2 .. 1 of the stage k = stage.
DEV void gft_sort_local_body(const GftDev *st, unsigned long long *ck, unsigned *ci, unsigned stage) {
  __shared__ unsigned long long sk[GFT_CHUNK];
  __shared__ unsigned si[GFT_CHUNK];
  const unsigned n = (unsigned)st->num_cand, np = gft_padded((int)n), tid = threadIdx.x;
  if (n == 0 || stage > np) return;
  for (unsigned c0 = blockIdx.x * GFT_CHUNK; c0 < np; c0 += gridDim.x * GFT_CHUNK) {  // (workgroup-uniform)
    for (unsigned i = tid; i < GFT_CHUNK; i += GFT_SORT_THREADS) {
      const bool in = stage != 0 || c0 + i < n;
      sk[i] = in ? ck[c0 + i] : 0ull, si[i] = in ? ci[c0 + i] : 0u;
    }
    __syncthreads();
    for (unsigned k = stage ? stage : 2u; k <= (stage ? stage : (unsigned)GFT_CHUNK); k <<= 1) {
      for (unsigned j = min(k >> 1, (unsigned)GFT_CHUNK / 2); j > 0; j >>= 1) {
        for (unsigned t = tid; t < GFT_CHUNK / 2; t += GFT_SORT_THREADS) {
          const unsigned a = gft_lower(t, j), b = a | j;
          const bool desc = ((c0 + a) & k) == 0;
          const unsigned long long ka = sk[a], kb = sk[b];
          const unsigned ia = si[a], ib = si[b];
          if (desc ? gft_before(kb, ib, ka, ia) : gft_before(ka, ia, kb, ib)) sk[a] = kb, sk[b] = ka, si[a] = ib, si[b] = ia;
        }
        __syncthreads();
      }
    }
    for (unsigned i = tid; i < GFT_CHUNK; i += GFT_SORT_THREADS) ck[c0 + i] = sk[i], ci[c0 + i] = si[i];
    __syncthreads();
  }
}
__global__ __launch_bounds__(GFT_SORT_THREADS) void k_gft_sort_local(const GftDev *st, unsigned long long *ck, unsigned *ci, unsigned stage) {
  gft_sort_local_body(st, ck, ci, stage);
}

// the step at distance j >= GFT_CHUNK of the stage k
DEV void gft_sort_global_body(const GftDev *st, unsigned long long *ck, unsigned *ci, unsigned k, unsigned j) {
  const unsigned n = (unsigned)st->num_cand, np = gft_padded((int)n);
  if (n == 0 || k > np) return;
  for (unsigned t = blockIdx.x * GFT_THREADS + threadIdx.x; t < np / 2; t += gridDim.x * GFT_THREADS) {
    const unsigned a = gft_lower(t, j), b = a | j;
    const bool desc = (a & k) == 0;
    const unsigned long long ka = ck[a], kb = ck[b];
    const unsigned ia = ci[a], ib = ci[b];
    if (desc ? gft_before(kb, ib, ka, ia) : gft_before(ka, ia, kb, ib)) ck[a] = kb, ck[b] = ka, ci[a] = ib, ci[b] = ia;
  }
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_sort_global(const GftDev *st, unsigned long long *ck, unsigned *ci, unsigned k, unsigned j) {
  gft_sort_global_body(st, ck, ci, k, j);
}

DEV void gft_pick_body(const GftDev *st, const unsigned *ci, int W, int d, int max_count, float *corners, LfvioGftOut *out) {
  __shared__ int s_acc[GFT_LIST];
  __shared__ int s_batch[GFT_THREADS];
  const int nk = st->num_kept, budget = max_count - nk, n = budget > 0 ? st->num_cand : 0;
  const int got = gft_greedy(
      n, d * d, budget,
      [&](int p) {
        const unsigned at = ci[p];
        return gft_pack((int)(at % (unsigned)W), (int)(at / (unsigned)W));
      },
      [&](int slot, int p, int v) { corners[2 * slot] = (float)(v & 0xffff), corners[2 * slot + 1] = (float)(v >> 16); }, s_acc, s_batch);
  if (threadIdx.x == 0) {
    out->num_kept = nk, out->num_corners = got, out->num_candidates = n;
    out->max_response = budget > 0 ? __longlong_as_double((long long)st->max_bits) : 0.0;
  }
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_pick(const GftDev *st, const unsigned *ci, int W, int d, int max_count, float *corners, LfvioGftOut *out) {
  gft_pick_body(st, ci, W, d, max_count, corners, out);
}
