// kernels_pnp.h — PnpSolver::compute_pose (vins_estimator/src/pnp_solver.cpp), the EPnP on bearing vectors that poses the
// non-keyframes of initialStructure() (estimator.cpp:288-357), with set_internal_parameters(0, 0, 1, 1).
//
//   k_pnp : grid F x 256, one workgroup per frame of a CSR of correspondences
//     1  means and the 3 x 3 moment of the world points (block sums), its Jacobi SVD, the control points        :45-75
//     2  barycentric coordinates per correspondence (kept in a device array), the 40 distinct sums of M^T M      :76-96, :313-330
//     3  wave 0: Jacobi from dev_smallmat.h on the 12 x 12 M^T M, lane r holding row r; the four smallest vectors :331-333
//     4  waves 0 - 2: L_6x10, rho, find_betas_<wave>, 15 Gauss-Newton steps (every lane the same numbers)        :101-230, :388-440
//     5  all threads, the three candidates side by side: pcs, their mean, solve_for_sign, W, R = U V^T, T,
//        reprojection_error (block sums)                                                                        :231-296
//     6  thread 0: the winner (:355-369), the finiteness gate, the record
//
// Every sum over correspondences is a block sum in a fixed order: a frame's bits do not depend on the other frames of the
// launch.  M^T M: row pair i of M is [a_j, 0, a_j x] / [0, a_j, a_j y] with x = (0 - u_0) / u_2, y = (0 - u_1) / u_2, so
// the 78 entries of the upper triangle are the 4 x 10 sums of a_j a_k {1, x, y, x^2 + y^2} and zeros.
// The column-pivoted Householder solve restates Eigen's ColPivHouseholderQR (norm downdating, the rank threshold on the
// largest remaining column norm, zeros for the dropped components); columns move by compare-exchange, never by a computed
// index (which would put the matrix in scratch memory).
#pragma once
#include "dev_smallmat.h"

constexpr int PNP_THREADS = 256, PNP_MIN_POINTS = 6, PNP_MAX_POINTS = 4096;

struct PnpRecord {  // LfvioPnpOut, as the kernel writes it
  int status, chosen;
  double R[9], T[3], err[3];
};

// x = A.colPivHouseholderQr().solve(b) for a 6 x NC matrix (Eigen/src/QR/ColPivHouseholderQR.h, computeInPlace and
// _solve_impl), thread-private and fully unrolled.
template <int NC>
DEV void pnp_colpiv_solve(double (&A)[6][NC], double (&b)[6], double (&x)[NC]) {
  constexpr int NR = 6;
  const double eps = 2.220446049250313e-16, downdate_thr = 1.4901161193847656e-08;  // sqrt(eps)
  double nu[NC], nd[NC], hc[NC];
  int perm[NC];
  double maxn = 0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    double s = 0;
#pragma unroll
    for (int r = 0; r < NR; r++) s += A[r][c] * A[r][c];
    nu[c] = nd[c] = sqrt(s), perm[c] = c;
    maxn = fmax(maxn, nu[c]);
  }
  const double thr_helper = (maxn * eps) * (maxn * eps) / (double)NR;
  int nonzero = NC;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    int big = k;
    double bn = nu[k];
#pragma unroll
    for (int c = k + 1; c < NC; c++)
      if (nu[c] > bn) bn = nu[c], big = c;
    if (nonzero == NC && bn * bn < thr_helper * (double)(NR - k)) nonzero = k;
#pragma unroll
    for (int c = k + 1; c < NC; c++) {
      const bool sw = big == c;
      cswap(sw, nu[k], nu[c]), cswap(sw, nd[k], nd[c]), cswap(sw, perm[k], perm[c]);
#pragma unroll
      for (int r = 0; r < NR; r++) cswap(sw, A[r][k], A[r][c]);
    }
    // makeHouseholderInPlace on rows k .. 5 of column k
    double tail = 0;
#pragma unroll
    for (int r = k + 1; r < NR; r++) tail += A[r][k] * A[r][k];
    const double c0 = A[k][k];
    double beta, tau;
    if (tail <= 2.2250738585072014e-308) {
      tau = 0.0, beta = c0;
#pragma unroll
      for (int r = k + 1; r < NR; r++) A[r][k] = 0.0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
#pragma unroll
      for (int r = k + 1; r < NR; r++) A[r][k] = A[r][k] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    A[k][k] = beta, hc[k] = tau;
#pragma unroll
    for (int c = k + 1; c < NC; c++) {  // applyHouseholderOnTheLeft
      double t = A[k][c];
#pragma unroll
      for (int r = k + 1; r < NR; r++) t += A[r][k] * A[r][c];
      A[k][c] -= tau * t;
#pragma unroll
      for (int r = k + 1; r < NR; r++) A[r][c] -= tau * A[r][k] * t;
    }
#pragma unroll
    for (int c = k + 1; c < NC; c++)
      if (nu[c] != 0.0) {
        double t = fabs(A[k][c]) / nu[c];
        t = (1.0 + t) * (1.0 - t);
        t = t < 0.0 ? 0.0 : t;
        const double q = nu[c] / nd[c], t2 = t * (q * q);
        if (t2 <= downdate_thr) {
          double s = 0;
#pragma unroll
          for (int r = k + 1; r < NR; r++) s += A[r][c] * A[r][c];
          nd[c] = sqrt(s), nu[c] = nd[c];
        } else {
          nu[c] *= sqrt(t);
        }
      }
  }
  // c = Q^T b over the first `nonzero` reflectors, the triangle of that size, zeros elsewhere
#pragma unroll
  for (int k = 0; k < NC; k++)
    if (k < nonzero) {
      double t = b[k];
#pragma unroll
      for (int r = k + 1; r < NR; r++) t += A[r][k] * b[r];
      b[k] -= hc[k] * t;
#pragma unroll
      for (int r = k + 1; r < NR; r++) b[r] -= hc[k] * A[r][k] * t;
    }
  double y[NC];
#pragma unroll
  for (int i = NC - 1; i >= 0; i--) {
    double s = b[i];
#pragma unroll
    for (int c = i + 1; c < NC; c++)
      if (c < nonzero) s -= A[i][c] * y[c];
    y[i] = i < nonzero ? s / A[i][i] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < NC; j++) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NC; i++) v = perm[i] == j ? y[i] : v;
    x[j] = v;
  }
}

// gauss_newton (:388-440): exactly 15 steps, no convergence test
DEV void pnp_gauss_newton(const double (&L)[6][10], const double (&rho)[6], double (&be)[4]) {
  for (int it = 0; it < 15; it++) {
    double A[6][4], b[6], x[4];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const double *l = L[i];
      A[i][0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
      A[i][1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
      A[i][2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
      A[i][3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
      b[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                       l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
    }
    pnp_colpiv_solve<4>(A, b, x);
#pragma unroll
    for (int i = 0; i < 4; i++) be[i] += x[i];
  }
}

// wave 0: the eigenvectors of the four smallest eigenvalues of the symmetric 12 x 12 G (lane r < 12 passes row r, the other
// lanes zeros), smallest first, by jacobi_wave's G V = B: |column c of B| = |lambda_c|, column c of V its vector.
// Lane r < 12 writes ut[i][r].
DEV void pnp_null4(double (&G)[12], int lane, double (*ut)[12]) {
  double W[12], n2[12];
  jacobi_wave<12>(G, W, n2, lane);
  unsigned taken = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double bn = 0, vv = 0;
    int bi = -1;
#pragma unroll
    for (int c = 0; c < 12; c++)
      if (!((taken >> c) & 1u) && (bi < 0 || n2[c] < bn)) bn = n2[c], vv = W[c], bi = c;
    taken |= 1u << bi;
    if (lane < 12) ut[i][lane] = vv;
  }
}

// SVD of a 3 x 3 W as W V = B; returns U V^T (:277-282, no determinant fix: the third left vector is the cross product of
// the other two with the sign of its own column of B, which is what its normalised column is wherever that is defined).
DEV m33 pnp_uvt(double (&B)[3][3]) {
  double V[3][3], n2[3];
  d3 u1, u2, u3;
  svd3_sorted(B, V, n2);
  svd3_u(B, n2, u1, u2, u3);
  if (u3.x * B[0][2] + u3.y * B[1][2] + u3.z * B[2][2] < 0.0) u3 = -u3;
  const double U1[3] = {u1.x, u1.y, u1.z}, U2[3] = {u2.x, u2.y, u2.z}, U3[3] = {u3.x, u3.y, u3.z};
  m33 R;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R.a[3 * i + j] = U1[i] * V[j][0] + U2[i] * V[j][1] + U3[i] * V[j][2];
  return R;
}

// The sign of a principal axis of the world points: its largest component (the first of equal ones) positive.  The control
// points depend on these signs and, with noisy bearings, the pose on the control points at the level of the noise, so this
// one sign cannot be left to the SVD (include/lfvio.h, deviation 2).
DEV d3 pnp_pin_axis(d3 v) {
  const double ax = fabs(v.x), ay = fabs(v.y), az = fabs(v.z);
  const double lead = (ax >= ay && ax >= az) ? v.x : (ay >= az ? v.y : v.z);
  return lead < 0.0 ? -v : v;
}

// compute_pose for the n correspondences (pw, us) of one frame, by the PNP_THREADS threads of one workgroup: steps 1 - 6 of
// the list above.  al: device array of 4 doubles per correspondence, written and read by the same thread (plus row 0 by
// everybody, behind a barrier).  red [40 * PNP_THREADS / 64], ut and sbeta are LDS blocks of the caller; thread 0 writes *out.
// k_pnp calls it once per workgroup, k_sfm_chain (kernels_sfmchain.h) once per solveFrameByPnP of its schedule.
DEV void pnp_pose(int n, const double *pw, const double *us, double *al, PnpRecord *out, double *red, double (*ut)[12], double (*sbeta)[4], int tid) {
  constexpr int NT = PNP_THREADS;
  const double dn = (double)n;

  // 1 ---- choose_control_points
  double s3[3] = {0, 0, 0};
  for (int i = tid; i < n; i += NT) {
    const d3 p = ld3(pw + 3 * (size_t)i);
    s3[0] += p.x, s3[1] += p.y, s3[2] += p.z;
  }
  block_sum_n<NT, 3>(s3, red, tid);
  const d3 c0 = mk3(s3[0] / dn, s3[1] / dn, s3[2] / dn);  // cws.row(0); also pw0 of estimate_R_and_t (:265-268)
  double s6[6] = {0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += NT) {
    const d3 p = ld3(pw + 3 * (size_t)i) - c0;
    s6[0] += p.x * p.x, s6[1] += p.x * p.y, s6[2] += p.x * p.z, s6[3] += p.y * p.y, s6[4] += p.y * p.z, s6[5] += p.z * p.z;
  }
  block_sum_n<NT, 6>(s6, red, tid);
  m33 CC;  // column j: cws.row(j + 1) - cws.row(0), as :82 forms it
  d3 cw[4];
  {
    double B[3][3] = {{s6[0], s6[1], s6[2]}, {s6[1], s6[3], s6[4]}, {s6[2], s6[4], s6[5]}}, V[3][3], n2[3];
    svd3_sorted(B, V, n2);
    cw[0] = c0;
    const d3 v[3] = {pnp_pin_axis(mk3(V[0][0], V[1][0], V[2][0])), pnp_pin_axis(mk3(V[0][1], V[1][1], V[2][1])), pnp_pin_axis(mk3(V[0][2], V[1][2], V[2][2]))};
    const double k[3] = {sqrt(sqrt(n2[0]) / dn), sqrt(sqrt(n2[1]) / dn), sqrt(sqrt(n2[2]) / dn)};
#pragma unroll
    for (int j = 0; j < 3; j++) {
      cw[j + 1] = c0 + k[j] * v[j];
      const d3 dlt = cw[j + 1] - c0;
      CC.a[j] = dlt.x, CC.a[3 + j] = dlt.y, CC.a[6 + j] = dlt.z;
    }
  }
  const m33 CI = inv33(CC);

  // 2 ---- compute_barycentric_coordinates, M^T M
  double acc[40];
#pragma unroll
  for (int k = 0; k < 40; k++) acc[k] = 0;
  for (int i = tid; i < n; i += NT) {
    const d3 p = ld3(pw + 3 * (size_t)i), u = ld3(us + 3 * (size_t)i);
    const double dx = p.x - c0.x, dy = p.y - c0.y, dz = p.z - c0.z;
    double a[4];
    a[1] = CI.a[0] * dx + CI.a[1] * dy + CI.a[2] * dz;
    a[2] = CI.a[3] * dx + CI.a[4] * dy + CI.a[5] * dz;
    a[3] = CI.a[6] * dx + CI.a[7] * dy + CI.a[8] * dz;
    a[0] = 1.0 - a[1] - a[2] - a[3];
    double *ai = al + 4 * (size_t)i;
    ai[0] = a[0], ai[1] = a[1], ai[2] = a[2], ai[3] = a[3];
    const double x = (0.0 - u.x) / u.z, y = (0.0 - u.y) / u.z, w = x * x + y * y;
    int k = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int l = j; l < 4; l++, k++) {
        const double pr = a[j] * a[l];
        acc[k] += pr, acc[10 + k] += pr * x, acc[20 + k] += pr * y, acc[30 + k] += pr * w;
      }
  }
  block_sum_n<NT, 40>(acc, red, tid);

  // 3 ---- the four smallest eigenvectors of M^T M
  if (tid < 64) {
    double G[12];
#pragma unroll
    for (int c = 0; c < 12; c++) G[c] = 0.0;
    // entry (3 j + a, 3 l + b) of M^T M: S1 at (0,0) and (1,1), Sx at (0,2) and (2,0), Sy at (1,2) and (2,1), Sw at (2,2)
    int k = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int l = j; l < 4; l++, k++) {
        const double S1 = acc[k], Sx = acc[10 + k], Sy = acc[20 + k], Sw = acc[30 + k];
#pragma unroll
        for (int t = 0; t < 2; t++) {  // the block (j, l) and its mirror (l, j)
          const int rj = t == 0 ? j : l, cl = t == 0 ? l : j;
          if (t == 1 && j == l) continue;
          if (tid == 3 * rj) G[3 * cl] = S1, G[3 * cl + 2] = Sx;
          if (tid == 3 * rj + 1) G[3 * cl + 1] = S1, G[3 * cl + 2] = Sy;
          if (tid == 3 * rj + 2) G[3 * cl] = Sx, G[3 * cl + 1] = Sy, G[3 * cl + 2] = Sw;
        }
      }
    pnp_null4(G, tid, ut);
  }
  __syncthreads();

  // 4 ---- L_6x10, rho, the three find_betas and their Gauss-Newton, one candidate per wave
  const int wave = tid >> 6;
  if (wave < 3) {
    double L[6][10], rho[6];
    {
      double dv[4][6][3];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        int a = 0, b = 1;
#pragma unroll
        for (int j = 0; j < 6; j++) {
#pragma unroll
          for (int k = 0; k < 3; k++) dv[i][j][k] = ut[i][3 * a + k] - ut[i][3 * b + k];
          if (++b > 3) a++, b = a + 1;
        }
      }
      auto dot3 = [](const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
#pragma unroll
      for (int i = 0; i < 6; i++) {
        L[i][0] = dot3(dv[0][i], dv[0][i]);
        L[i][1] = 2.0 * dot3(dv[0][i], dv[1][i]);
        L[i][2] = dot3(dv[1][i], dv[1][i]);
        L[i][3] = 2.0 * dot3(dv[0][i], dv[2][i]);
        L[i][4] = 2.0 * dot3(dv[1][i], dv[2][i]);
        L[i][5] = dot3(dv[2][i], dv[2][i]);
        L[i][6] = 2.0 * dot3(dv[0][i], dv[3][i]);
        L[i][7] = 2.0 * dot3(dv[1][i], dv[3][i]);
        L[i][8] = 2.0 * dot3(dv[2][i], dv[3][i]);
        L[i][9] = dot3(dv[3][i], dv[3][i]);
      }
      int a = 0, b = 1;
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const d3 d = cw[a] - cw[b];
        rho[j] = d.x * d.x + d.y * d.y + d.z * d.z;
        if (++b > 3) a++, b = a + 1;
      }
    }
    double be[4], rb[6];
#pragma unroll
    for (int i = 0; i < 6; i++) rb[i] = rho[i];
    if (wave == 0) {  // find_betas_0 (:145-172)
      double A[6][4], x[4];
#pragma unroll
      for (int i = 0; i < 6; i++) A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][3], A[i][3] = L[i][6];
      pnp_colpiv_solve<4>(A, rb, x);
      if (x[0] < 0) {
        be[0] = sqrt(-x[0]), be[1] = -x[1] / be[0], be[2] = -x[2] / be[0], be[3] = -x[3] / be[0];
      } else {
        be[0] = sqrt(x[0]), be[1] = x[1] / be[0], be[2] = x[2] / be[0], be[3] = x[3] / be[0];
      }
    } else if (wave == 1) {  // find_betas_1 (:174-201)
      double A[6][3], x[3];
#pragma unroll
      for (int i = 0; i < 6; i++) A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][2];
      pnp_colpiv_solve<3>(A, rb, x);
      if (x[0] < 0) {
        be[0] = sqrt(-x[0]), be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0;
      } else {
        be[0] = sqrt(x[0]), be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) be[0] = -be[0];
      be[2] = 0.0, be[3] = 0.0;
    } else {  // find_betas_2 (:202-230); :226-227 changes B5[0] after its last use and has no effect
      double A[6][5], x[5];
#pragma unroll
      for (int i = 0; i < 6; i++) A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][2], A[i][3] = L[i][3], A[i][4] = L[i][4];
      pnp_colpiv_solve<5>(A, rb, x);
      if (x[0] < 0) {
        be[0] = sqrt(-x[0]), be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0;
      } else {
        be[0] = sqrt(x[0]), be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0;
      }
      be[2] = x[3] / be[0], be[3] = 0.0;
    }
    pnp_gauss_newton(L, rho, be);
    if ((tid & 63) == 0) sbeta[wave][0] = be[0], sbeta[wave][1] = be[1], sbeta[wave][2] = be[2], sbeta[wave][3] = be[3];
  }
  __syncthreads();

  // 5 ---- compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error: three candidates side by side
  d3 cc[3][4];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double v[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += sbeta[c][i] * ut[i][3 * j + k];
      cc[c][j] = mk3(v[0], v[1], v[2]);
    }
  {
    const double a0 = al[0], a1 = al[1], a2 = al[2], a3 = al[3], sign0 = us[2] > 0 ? 1.0 : -1.0;  // (:32-39, :249)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double z = a0 * cc[c][0].z + a1 * cc[c][1].z + a2 * cc[c][2].z + a3 * cc[c][3].z;
      if ((z < 0.0 && sign0 > 0) || (z > 0.0 && sign0 < 0))
#pragma unroll
        for (int j = 0; j < 4; j++) cc[c][j] = -cc[c][j];
    }
  }
  double s9[9];
#pragma unroll
  for (int k = 0; k < 9; k++) s9[k] = 0;
  for (int i = tid; i < n; i += NT) {
    const double *ai = al + 4 * (size_t)i;
    const double a0 = ai[0], a1 = ai[1], a2 = ai[2], a3 = ai[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      s9[3 * c] += a0 * cc[c][0].x + a1 * cc[c][1].x + a2 * cc[c][2].x + a3 * cc[c][3].x;
      s9[3 * c + 1] += a0 * cc[c][0].y + a1 * cc[c][1].y + a2 * cc[c][2].y + a3 * cc[c][3].y;
      s9[3 * c + 2] += a0 * cc[c][0].z + a1 * cc[c][1].z + a2 * cc[c][2].z + a3 * cc[c][3].z;
    }
  }
  block_sum_n<NT, 9>(s9, red, tid);
  d3 pc0[3];
#pragma unroll
  for (int c = 0; c < 3; c++) pc0[c] = mk3(s9[3 * c] / dn, s9[3 * c + 1] / dn, s9[3 * c + 2] / dn);
  double w27[27];
#pragma unroll
  for (int k = 0; k < 27; k++) w27[k] = 0;
  for (int i = tid; i < n; i += NT) {
    const double *ai = al + 4 * (size_t)i;
    const double a0 = ai[0], a1 = ai[1], a2 = ai[2], a3 = ai[3];
    const d3 q = ld3(pw + 3 * (size_t)i) - c0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const d3 p = mk3(a0 * cc[c][0].x + a1 * cc[c][1].x + a2 * cc[c][2].x + a3 * cc[c][3].x,
                       a0 * cc[c][0].y + a1 * cc[c][1].y + a2 * cc[c][2].y + a3 * cc[c][3].y,
                       a0 * cc[c][0].z + a1 * cc[c][1].z + a2 * cc[c][2].z + a3 * cc[c][3].z) - pc0[c];
      double *w = w27 + 9 * c;
      w[0] += p.x * q.x, w[1] += p.x * q.y, w[2] += p.x * q.z;
      w[3] += p.y * q.x, w[4] += p.y * q.y, w[5] += p.y * q.z;
      w[6] += p.z * q.x, w[7] += p.z * q.y, w[8] += p.z * q.z;
    }
  }
  block_sum_n<NT, 27>(w27, red, tid);
  m33 R[3];
  d3 T[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double B[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) B[i][j] = w27[9 * c + 3 * i + j];
    R[c] = pnp_uvt(B);
    const double *r = R[c].a;
    T[c] = pc0[c] - mk3(r[0] * c0.x + r[1] * c0.y + r[2] * c0.z, r[3] * c0.x + r[4] * c0.y + r[5] * c0.z, r[6] * c0.x + r[7] * c0.y + r[8] * c0.z);
  }
  double e3[3] = {0, 0, 0};
  for (int i = tid; i < n; i += NT) {
    const d3 p = ld3(pw + 3 * (size_t)i), u = ld3(us + 3 * (size_t)i);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double *r = R[c].a;
      const double x = u.x - ((r[0] * p.x + r[1] * p.y + r[2] * p.z) + T[c].x), y = u.y - ((r[3] * p.x + r[4] * p.y + r[5] * p.z) + T[c].y),
                   z = u.z - ((r[6] * p.x + r[7] * p.y + r[8] * p.z) + T[c].z);
      e3[c] += x * x + y * y + z * z;
    }
  }
  block_sum_n<NT, 3>(e3, red, tid);

  // 6 ---- the winner (:355-369: strict <, the first candidate wins a tie) and the record
  if (tid == 0) {
    const double e0 = e3[0] / dn, e1 = e3[1] / dn, e2 = e3[2] / dn;
    const bool one = e1 < e0;
    const bool two = e2 < (one ? e1 : e0);
    const int N = two ? 2 : one ? 1 : 0;
    bool finite = isfinite(e0) && isfinite(e1) && isfinite(e2);
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const double v = two ? R[2].a[j] : one ? R[1].a[j] : R[0].a[j];
      finite = finite && isfinite(v);
      out->R[j] = v;
    }
    const d3 t = mk3(two ? T[2].x : one ? T[1].x : T[0].x, two ? T[2].y : one ? T[1].y : T[0].y, two ? T[2].z : one ? T[1].z : T[0].z);
    finite = finite && isfinite(t.x) && isfinite(t.y) && isfinite(t.z);
    out->T[0] = t.x, out->T[1] = t.y, out->T[2] = t.z;
    out->err[0] = e0, out->err[1] = e1, out->err[2] = e2;
    out->chosen = N, out->status = finite ? 0 : 1;
  }
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp(const int *offset, const double *pw_all, const double *us_all, double *alpha_all,
                                                     PnpRecord *out_all) {
  __shared__ double red[40 * PNP_THREADS / 64], ut[4][12], sbeta[3][4];
  const int f = blockIdx.x, o = offset[f], n = offset[f + 1] - o;
  pnp_pose(n, pw_all + 3 * (size_t)o, us_all + 3 * (size_t)o, alpha_all + 4 * (size_t)o, out_all + f, red, ut, sbeta, threadIdx.x);
}
