// dev_smallmat.h — the small dense algebra the feature, two-view and PnP kernels share: a one-sided Jacobi (thread-private
// and wave-wide), the sorted SVD of a 3 x 3 built on it, and compare-exchange.
#pragma once
#include "dev_math.h"

// One Jacobi rotation: where columns with squared norms al, be and inner product ga are not orthogonal to within tol,
// apply(c, s) with the (c, s) that make them so.  (A callable keeps the test, c, s and their use in one branch.)
template <class F>
DEV void jacobi_rot(double al, double be, double ga, double tol, F apply) {
  if (ga == 0.0 || fabs(ga) <= tol * sqrt(al * be)) return;
  const double zeta = (be - al) / (2.0 * ga);
  const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  apply(c, s);
}

// One-sided Jacobi on a matrix with NR rows and NC columns held in registers: B <- B V with orthogonal columns.  Thread-
// private and fully unrolled (every index is a compile-time constant); at most 30 sweeps.  It works on copies of its own:
// an array reached through a reference is kept as one vector value after inlining, and every branch then moves all of it
// (without the copies k_tv_fit has 15 720 instructions, with them 14 907; tools/isa_census.py or tools/kres.py re-check it).
template <int NR, int NC>
DEV void jacobi_cols(double (&B)[NR][NC], double (&V)[NC][NC], double tol) {
  double b[NR][NC], v[NC][NC];
#pragma unroll
  for (int i = 0; i < NR * NC; i++) b[i / NC][i % NC] = B[i / NC][i % NC];
#pragma unroll
  for (int i = 0; i < NC * NC; i++) v[i / NC][i % NC] = i / NC == i % NC ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < NC - 1; p++)
#pragma unroll
      for (int q = p + 1; q < NC; q++) {
        double al = 0, be = 0, ga = 0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
          const double x = b[r][p], y = b[r][q];
          al += x * x, be += y * y, ga += x * y;
        }
        jacobi_rot(al, be, ga, tol, [&](double c, double s) {
          rotated = true;
#pragma unroll
          for (int r = 0; r < NR; r++) {
            const double x = b[r][p], y = b[r][q];
            b[r][p] = c * x - s * y;
            b[r][q] = s * x + c * y;
          }
#pragma unroll
          for (int r = 0; r < NC; r++) {
            const double x = v[r][p], y = v[r][q];
            v[r][p] = c * x - s * y;
            v[r][q] = s * x + c * y;
          }
        });
      }
    if (!rotated) break;
  }
#pragma unroll
  for (int i = 0; i < NR * NC; i++) B[i / NC][i % NC] = b[i / NC][i % NC];
#pragma unroll
  for (int i = 0; i < NC * NC; i++) V[i / NC][i % NC] = v[i / NC][i % NC];
}

// The same on an N x N matrix spread over a wave: lane r < N passes row r of G (the other lanes zeros) and gets row r of
// G V and of V (in W); n2: the squared column norms of G V, the same in every lane.  The tolerance is fixed at 2.3e-16.
// Working copies as in jacobi_cols.
template <int N>
DEV void jacobi_wave(double (&G)[N], double (&W)[N], double (&n2)[N], int lane) {
  double g[N], w[N];
#pragma unroll
  for (int c = 0; c < N; c++) g[c] = G[c], w[c] = c == lane ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; p++)
#pragma unroll
      for (int q = p + 1; q < N; q++) {
        const double al = wave_sum(g[p] * g[p]), be = wave_sum(g[q] * g[q]), ga = wave_sum(g[p] * g[q]);
        jacobi_rot(al, be, ga, 2.3e-16, [&](double c, double s) {
          rotated = true;
          const double x = g[p], y = g[q], vx = w[p], vy = w[q];
          g[p] = c * x - s * y, g[q] = s * x + c * y;
          w[p] = c * vx - s * vy, w[q] = s * vx + c * vy;
        });
      }
    if (!rotated) break;
  }
#pragma unroll
  for (int c = 0; c < N; c++) G[c] = g[c], W[c] = w[c], n2[c] = wave_sum(g[c] * g[c]);
}

template <class T>
DEV void cswap(bool c, T &a, T &b) {
  const T x = c ? b : a, y = c ? a : b;
  a = x, b = y;
}

// Columns P and Q of B, V and n2 into falling order of n2.  (Whole columns move by compare-exchange: picking a column by a
// computed index puts B and V in scratch memory.)
template <int P, int Q>
DEV void sort_cols(double (&B)[3][3], double (&V)[3][3], double (&n2)[3]) {
  const bool c = n2[P] < n2[Q];
  cswap(c, n2[P], n2[Q]);
#pragma unroll
  for (int r = 0; r < 3; r++) cswap(c, B[r][P], B[r][Q]), cswap(c, V[r][P], V[r][Q]);
}
// SVD of a 3 x 3 as B <- B V (columns of B: sigma_c u_c), columns sorted by falling squared norm n2.
DEV void svd3_sorted(double (&B)[3][3], double (&V)[3][3], double (&n2)[3]) {
  jacobi_cols<3, 3>(B, V, 2.3e-16);
#pragma unroll
  for (int c = 0; c < 3; c++) n2[c] = B[0][c] * B[0][c] + B[1][c] * B[1][c] + B[2][c] * B[2][c];
  sort_cols<0, 1>(B, V, n2), sort_cols<1, 2>(B, V, n2), sort_cols<0, 1>(B, V, n2);
}

// The left vectors of svd3_sorted's result: the two leading columns normalised, and their cross product.
DEV void svd3_u(const double (&B)[3][3], const double (&n2)[3], d3 &u1, d3 &u2, d3 &u3) {
  const double is1 = 1.0 / sqrt(n2[0]), is2 = 1.0 / sqrt(n2[1]);
  u1 = is1 * mk3(B[0][0], B[1][0], B[2][0]), u2 = is2 * mk3(B[0][1], B[1][1], B[2][1]), u3 = cross(u1, u2);
}
