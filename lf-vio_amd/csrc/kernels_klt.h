// kernels_klt.h — pyramidal Lucas-Kanade (cv::calcOpticalFlowPyrLK as feature_tracker.cpp:127 calls it) behind lfvio_klt_track;
// the algorithm is stated in include/lfvio.h and, as the specification, in tests/klt_ref.py.
//
//   k_klt_down  : one level of the pyramid from the one below: [1 4 6 4 1] x [1 4 6 4 1], reflect-101, even pixels, (s + 128) >> 8.
//                 One thread per output pixel, integers only: a level is exact.  One launch per level.
//   k_klt_track : one workgroup of 256 per point walks the levels from levels_used down to 0 in one launch.  Per level the
//                 (win + 3)^2 pixels around the window come into LDS once (reflect-101 outside the level); the bilinear patches of I
//                 and of both Scharr gradients (taken from those pixels: no derivative image exists) stay in LDS as floats for the
//                 level's iterations; J is sampled from the level in global memory.  Positions, weights, the five sums of an
//                 iteration and the 2 x 2 solve are doubles; the sums are reduced in a fixed order (block_sum_n: inside the wave,
//                 then the four waves in order), so every thread holds the same bits, every branch on them is workgroup-uniform, and
//                 a point's result depends neither on N nor on its index.
#pragma once
#include "dev_math.h"
#include "klt_plan.h"

constexpr int KLT_THREADS = 256;
constexpr int KLT_RAW = KLT_MAX_WIN + 3;  // side of the staged pixel block: the window, one more for the bilinear taps, one each side for Scharr

struct KltArgs {
  int win, levels_used, max_level, max_iter, border;
  double eps2, min_eig;
  int w[KLT_LEVELS], h[KLT_LEVELS];
  long long off[KLT_LEVELS];
};

// index i of an axis of n >= 2 pixels continued by reflection about the centres of its end pixels, repeated while needed
DEV int klt_reflect(int i, int n) {
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// (the bodies are device functions: kernels_trackbatch.h runs the same code per slot)
DEV void klt_down_body(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const int k[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int i = 0; i < 5; i++) xs[i] = klt_reflect(2 * x - 2 + i, sw);
  int s = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const unsigned char *row = src + (size_t)klt_reflect(2 * y - 2 + j, sh) * sw;
    int t = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) t += k[i] * row[xs[i]];
    s += k[j] * t;
  }
  dst[(size_t)y * dw + x] = (unsigned char)((s + 128) >> 8);
}
__global__ __launch_bounds__(256) void k_klt_down(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh) {
  klt_down_body(src, sw, sh, dst, dw, dh);
}

// floor of a window's corner inside [-win, cols) x [-win, rows)?  (in doubles: a NaN or a huge coordinate is outside, and only an
// inside one is converted to int)
DEV bool klt_inside(double fx, double fy, int win, int cols, int rows) { return fx >= -win && fx < cols && fy >= -win && fy < rows; }

DEV void klt_track_body(const KltArgs &a, int N, const unsigned char *prev_pyr, const unsigned char *next_pyr, const float *pts, float *next,
                        unsigned char *status, int *iters) {
  __shared__ unsigned char raw[KLT_RAW * KLT_RAW];
  __shared__ float pI[KLT_MAX_WIN * KLT_MAX_WIN], pX[KLT_MAX_WIN * KLT_MAX_WIN], pY[KLT_MAX_WIN * KLT_MAX_WIN];
  __shared__ double red[5 * KLT_THREADS / 64];
  const int pt = blockIdx.x, tid = threadIdx.x;
  if (pt >= N) return;
  const int win = a.win, n_win = win * win, S = win + 3;
  const double half = (win - 1) * 0.5;
  // sample k = tid + 256 m of the window is (row, column) = (k / win, k % win): walked by steps instead of divisions
  const int r_first = tid / win, c_first = tid - r_first * win, r_step = KLT_THREADS / win, c_step = KLT_THREADS - r_step * win;
  const double px = (double)pts[2 * pt], py = (double)pts[2 * pt + 1];
  double gx = 0, gy = 0;  // the guess
  int st = 1;
  for (int L = a.levels_used; L >= 0; L--) {
    const int cols = a.w[L], rows = a.h[L];
    const unsigned char *I = prev_pyr + a.off[L], *J = next_pyr + a.off[L];
    const double sc = 1.0 / (double)(1 << L);
    const double prx = px * sc, pry = py * sc;
    if (L == a.levels_used) gx = prx, gy = pry;
    else gx *= 2.0, gy *= 2.0;
    int nit = 0;
    const double cx = prx - half, cy = pry - half, fx = floor(cx), fy = floor(cy);
    bool run = klt_inside(fx, fy, win, cols, rows);
    double A11 = 0, A12 = 0, A22 = 0, det = 0;
    if (run) {
      const int ix = (int)fx, iy = (int)fy;
      const double ax = cx - fx, ay = cy - fy;
      const double w00 = (1 - ax) * (1 - ay), w01 = ax * (1 - ay), w10 = (1 - ax) * ay, w11 = ax * ay;
      __syncthreads();  // (the level above is done with raw and the patches)
      for (int k = tid; k < S * S; k += KLT_THREADS) {  // raw[j][i] = pixel (ix - 1 + i, iy - 1 + j)
        const int j = k / S, i = k - j * S;
        raw[k] = I[(size_t)klt_reflect(iy - 1 + j, rows) * cols + klt_reflect(ix - 1 + i, cols)];
      }
      __syncthreads();
      double s[3] = {0, 0, 0};
      for (int k = tid, r = r_first, c = c_first; k < n_win; k += KLT_THREADS, r += r_step, c += c_step) {
        if (c >= win) c -= win, r++;
        double v[3][4];  // I, 32 gx, 32 gy at the four taps (c + dx, r + dy)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int dx = q & 1, dy = q >> 1;
          const unsigned char *o = raw + (r + dy + 1) * S + (c + dx + 1);
          const int x = ix + c + dx, y = iy + r + dy;
          const bool in = (unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows;  // outside the level both derivatives are 0
          const int sx = 3 * ((int)o[-S + 1] - (int)o[-S - 1]) + 10 * ((int)o[1] - (int)o[-1]) + 3 * ((int)o[S + 1] - (int)o[S - 1]);
          const int sy = 3 * ((int)o[S - 1] - (int)o[-S - 1]) + 10 * ((int)o[S] - (int)o[-S]) + 3 * ((int)o[S + 1] - (int)o[-S + 1]);
          v[0][q] = (double)o[0], v[1][q] = in ? sx / 32.0 : 0.0, v[2][q] = in ? sy / 32.0 : 0.0;
        }
        float f[3];
#pragma unroll
        for (int m = 0; m < 3; m++) f[m] = (float)(w00 * v[m][0] + w01 * v[m][1] + w10 * v[m][2] + w11 * v[m][3]);
        pI[k] = f[0], pX[k] = f[1], pY[k] = f[2];
        const double dxv = (double)f[1], dyv = (double)f[2];
        s[0] += dxv * dxv, s[1] += dxv * dyv, s[2] += dyv * dyv;
      }
      block_sum_n<KLT_THREADS, 3>(s, red, tid);  // (its barriers also publish the patches)
      A11 = s[0] / 1024.0, A12 = s[1] / 1024.0, A22 = s[2] / 1024.0;
      det = A11 * A22 - A12 * A12;
      const double min_eig = (A11 + A22 - sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (double)(2 * n_win);
      run = !(min_eig < a.min_eig || det < 1.1920928955078125e-07);
    }
    if (!run) {
      if (L == 0) st = 0;
    } else {
      double pdx = 0, pdy = 0;
      for (int j = 0; j < a.max_iter; j++) {
        const double qx = gx - half, qy = gy - half, hx = floor(qx), hy = floor(qy);
        if (!klt_inside(hx, hy, win, cols, rows)) {
          if (L == 0) st = 0;
          break;
        }
        const int jx = (int)hx, jy = (int)hy;
        const double bx = qx - hx, by = qy - hy;
        const double w00 = (1 - bx) * (1 - by), w01 = bx * (1 - by), w10 = (1 - bx) * by, w11 = bx * by;
        double b[2] = {0, 0};
        for (int k = tid, r = r_first, c = c_first; k < n_win; k += KLT_THREADS, r += r_step, c += c_step) {
          if (c >= win) c -= win, r++;
          const unsigned char *r0 = J + (size_t)klt_reflect(jy + r, rows) * cols, *r1 = J + (size_t)klt_reflect(jy + r + 1, rows) * cols;
          const int x0 = klt_reflect(jx + c, cols), x1 = klt_reflect(jx + c + 1, cols);
          // (J rounded to float like the I patch: an image tracked against itself gives exact zeros)
          const float jv = (float)(w00 * (double)r0[x0] + w01 * (double)r0[x1] + w10 * (double)r1[x0] + w11 * (double)r1[x1]);
          const double d = (double)jv - (double)pI[k];
          b[0] += d * (double)pX[k], b[1] += d * (double)pY[k];
        }
        block_sum_n<KLT_THREADS, 2>(b, red, tid);  // (its first barrier stands behind every thread's reads of the totals before)
        const double b1 = b[0] / 1024.0, b2 = b[1] / 1024.0;
        const double dx = (A12 * b2 - A22 * b1) / det, dy = (A12 * b1 - A11 * b2) / det;
        gx += dx, gy += dy;
        nit = j + 1;
        if (dx * dx + dy * dy <= a.eps2) break;
        if (j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
          gx -= dx * 0.5, gy -= dy * 0.5;
          break;
        }
        pdx = dx, pdy = dy;
      }
    }
    if (tid == 0 && iters) iters[(size_t)pt * (a.max_level + 1) + L] = nit;
  }
  if (tid == 0) {
    const float ox = (float)gx, oy = (float)gy;
    if (st && a.border >= 0) {
      const double rx = rint((double)ox), ry = rint((double)oy);  // half to even, like cvRound
      if (!(rx >= a.border && rx < a.w[0] - a.border && ry >= a.border && ry < a.h[0] - a.border)) st = 0;
    }
    next[2 * pt] = ox, next[2 * pt + 1] = oy;
    status[pt] = (unsigned char)st;
    if (iters)
      for (int L = a.levels_used + 1; L <= a.max_level; L++) iters[(size_t)pt * (a.max_level + 1) + L] = 0;
  }
}
__global__ __launch_bounds__(KLT_THREADS) void k_klt_track(KltArgs a, int N, const unsigned char *prev_pyr, const unsigned char *next_pyr,
                                                           const float *pts, float *next, unsigned char *status, int *iters) {
  klt_track_body(a, N, prev_pyr, next_pyr, pts, next, status, iters);
}
