// kernels_sfmba.h — the "full BA" that ends GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:233-309): ReprojectionError3D
// (initial_sfm.h:25-63) over F <= 11 frames and P <= 4096 points, minimised by Ceres' trust-region loop with the Levenberg-Marquardt
// strategy and DENSE_SCHUR, as DESIGN.md §3h restates it (tests/sfm_ba_ref.py is the same statement in numpy).
//
//   k_sfm_ba : ONE workgroup of 256 threads runs the whole loop; no host round trip, no other workgroup to wait for
//     linearise        a thread per point walks the point's observations: r, the 3 x 6 camera and 3 x 3 point Jacobians (kept per
//                      observation in device memory), the point's V and g; the cameras' U_f and g_f are block sums, one frame at a time
//     point blocks     a thread per point: the scaled, damped V, its inverse, W and Y = W V^-1 per observation
//     reduced system   6 F - 9 <= 57 columns in LDS, the right-hand side as one more row; a thread per entry walks the points in order
//     Cholesky         right-looking, a column per step, the rhs row riding along (the forward substitution), then the back-substitution
//     step             cameras from the solve, points by back-substitution, model cost change, candidate, candidate cost, decision
//
// Every sum is taken in a fixed order (block sums; the points in index order): a repeated call returns the same bits.  Every loop is
// bounded by the iteration cap or a size.  The tiled MFMA Cholesky of kernels_solve.h is built for a compile-time 172 and four
// waves' worth of 16 x 16 tiles; at <= 57 columns of a run-time count a plain column Cholesky in LDS is what fits.
#pragma once
#include "dev_math.h"
#include "../../include/lfvio.h"

constexpr int SFMBA_THREADS = 256, SFMBA_MAX_POINTS = 4096, SFMBA_MAX_COLS = 6 * LFVIO_NUM_FRAMES - 9, SFMBA_LD = SFMBA_MAX_COLS + 2;
constexpr int SFMBA_PW = 24;  // doubles per point: V[6] gp[3] Vinv[6] sp[3] gps[3] dp[3]
constexpr int SFMBA_OW = 66;  // doubles per observation: Jc[18] Jp[9] r[3] W[18] Y[18]
constexpr int PW_V = 0, PW_G = 6, PW_VI = 9, PW_S = 15, PW_GS = 18, PW_D = 21, OW_JC = 0, OW_JP = 18, OW_R = 27, OW_W = 30, OW_Y = 48;

struct SfmBaHead {
  int F, P, max_it, n;
  int col[LFVIO_NUM_FRAMES][6];  // column of the reduced system, or -1 for a constant one
  double ftol, gtol, ptol;
};
struct SfmBaResult {
  int nonfinite, pad;
  LfvioSfmBaOut o;
};

// QuaternionParameterization::Plus: [cos|d|, sin|d| / |d| d] (x) q; a zero delta leaves q as it is; no renormalisation
DEV q4 sfmba_plus(q4 q, d3 d) {
  const double nd = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
  if (!(nd > 0.0)) return q;
  const double s = sin(nd) / nd;
  return qmul(q4{cos(nd), s * d.x, s * d.y, s * d.z}, q);
}
// R(q / |q|) (ceres::QuaternionRotatePoint normalises first)
DEV m33 sfmba_R(q4 q) {
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const double w = q.w / n, x = q.x / n, y = q.y / n, z = q.z / n;
  m33 R;
  R.a[0] = 1 - 2 * (y * y + z * z), R.a[1] = 2 * (x * y - w * z), R.a[2] = 2 * (x * z + w * y);
  R.a[3] = 2 * (x * y + w * z), R.a[4] = 1 - 2 * (x * x + z * z), R.a[5] = 2 * (y * z - w * x);
  R.a[6] = 2 * (x * z - w * y), R.a[7] = 2 * (y * z + w * x), R.a[8] = 1 - 2 * (x * x + y * y);
  return R;
}
DEV double sfmba_clamp(double d) { return d < 1e-6 ? 1e-6 : (d > 1e32 ? 1e32 : d); }

__global__ __launch_bounds__(SFMBA_THREADS) void k_sfm_ba(const SfmBaHead *hd, const int *off, const int *frm, const int *slot, const double *bearing,
                                                           double *qio, double *tio, double *X, double *Xc, double *pw, double *ow, SfmBaResult *res) {
  constexpr int NT = SFMBA_THREADS, NF = LFVIO_NUM_FRAMES, LD = SFMBA_LD;
  __shared__ double S[(SFMBA_MAX_COLS + 1) * SFMBA_LD], red[42 * NT / 64], s_y[SFMBA_MAX_COLS];
  __shared__ double s_q[2][NF][4], s_t[2][NF][3], s_R[2][NF][9], s_sc[NF][6], s_U[NF][36], s_gc[NF][6], s_dc[NF][6];
  __shared__ int s_cf[SFMBA_MAX_COLS], s_ck[SFMBA_MAX_COLS];
  const int tid = threadIdx.x, F = hd->F, P = hd->P, n = hd->n, max_it = hd->max_it;
  const double ftol = hd->ftol, gtol = hd->gtol, ptol = hd->ptol;

  if (tid < F) {
#pragma unroll
    for (int k = 0; k < 4; k++) s_q[0][tid][k] = qio[4 * tid + k];
#pragma unroll
    for (int k = 0; k < 3; k++) s_t[0][tid][k] = tio[3 * tid + k];
    const m33 R = sfmba_R(q4{s_q[0][tid][0], s_q[0][tid][1], s_q[0][tid][2], s_q[0][tid][3]});
#pragma unroll
    for (int k = 0; k < 9; k++) s_R[0][tid][k] = R.a[k];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int c = hd->col[tid][k];
      if (c >= 0 && c < SFMBA_MAX_COLS) s_cf[c] = tid, s_ck[c] = k;
      s_dc[tid][k] = 0.0;
    }
  }
  __syncthreads();

  // ---- cost (and, with JAC, the Jacobians per observation and V, g per point) of state st (0: x, 1: the candidate); 1/2 sum r^2
  auto evaluate = [&](int st, bool jac) -> double {
    const double *Xs = st ? Xc : X;
    double cost = 0.0;
    for (int i = tid; i < P; i += NT) {
      const d3 Xi = ld3(Xs + 3 * (size_t)i);
      double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
      for (int o = off[i]; o < off[i + 1]; o++) {
        const int f = frm[o];
        const double *Rf = s_R[st][f], *tf = s_t[st][f];
        const d3 RX = mk3(Rf[0] * Xi.x + Rf[1] * Xi.y + Rf[2] * Xi.z, Rf[3] * Xi.x + Rf[4] * Xi.y + Rf[5] * Xi.z, Rf[6] * Xi.x + Rf[7] * Xi.y + Rf[8] * Xi.z);
        const d3 p = mk3(RX.x + tf[0], RX.y + tf[1], RX.z + tf[2]);
        const double nrm = sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
        const double ph[3] = {p.x / nrm, p.y / nrm, p.z / nrm};
        const double r[3] = {ph[0] - bearing[3 * (size_t)o], ph[1] - bearing[3 * (size_t)o + 1], ph[2] - bearing[3 * (size_t)o + 2]};
        cost += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        if (jac) {
          double *w = ow + (size_t)o * SFMBA_OW;
          double N[3][3];
#pragma unroll
          for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) N[a][b] = ((a == b ? 1.0 : 0.0) - ph[a] * ph[b]) / nrm;
          // -2 [R X]x
          const double Sx[3][3] = {{0.0, 2 * RX.z, -2 * RX.y}, {-2 * RX.z, 0.0, 2 * RX.x}, {2 * RX.y, -2 * RX.x, 0.0}};
          double Jp[3][3];
#pragma unroll
          for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++) {
              w[OW_JC + 6 * a + b] = N[a][0] * Sx[0][b] + N[a][1] * Sx[1][b] + N[a][2] * Sx[2][b];
              w[OW_JC + 6 * a + 3 + b] = N[a][b];
              Jp[a][b] = N[a][0] * Rf[b] + N[a][1] * Rf[3 + b] + N[a][2] * Rf[6 + b];
              w[OW_JP + 3 * a + b] = Jp[a][b];
            }
            w[OW_R + a] = r[a];
          }
          int k = 0;
#pragma unroll
          for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = a; b < 3; b++, k++) V[k] += Jp[0][a] * Jp[0][b] + Jp[1][a] * Jp[1][b] + Jp[2][a] * Jp[2][b];
            g[a] += Jp[0][a] * r[0] + Jp[1][a] * r[1] + Jp[2][a] * r[2];
          }
        }
      }
      if (jac) {
        double *q = pw + (size_t)i * SFMBA_PW;
#pragma unroll
        for (int k = 0; k < 6; k++) q[PW_V + k] = V[k];
#pragma unroll
        for (int k = 0; k < 3; k++) q[PW_G + k] = g[k];
      }
    }
    return 0.5 * block_sum<NT>(cost, red, tid);
  };

  // ---- U_f = sum Jc^T Jc and g_f = sum Jc^T r of every frame (unscaled), each a block sum over the points
  auto camera_blocks = [&]() {
    for (int f = 0; f < F; f++) {
      double acc[27];
#pragma unroll
      for (int k = 0; k < 27; k++) acc[k] = 0.0;
      for (int i = tid; i < P; i += NT) {
        const int o = slot[(size_t)i * F + f];
        if (o < 0) continue;
        const double *w = ow + (size_t)o * SFMBA_OW;
        double J[3][6], r[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
          for (int b = 0; b < 6; b++) J[a][b] = w[OW_JC + 6 * a + b];
          r[a] = w[OW_R + a];
        }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
          for (int b = a; b < 6; b++, k++) acc[k] += J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b];
          acc[21 + a] += J[0][a] * r[0] + J[1][a] * r[1] + J[2][a] * r[2];
        }
      }
      block_sum_n<NT, 27>(acc, red, tid);
      if (tid == 0) {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
          for (int b = a; b < 6; b++, k++) s_U[f][6 * a + b] = acc[k], s_U[f][6 * b + a] = acc[k];
          s_gc[f][a] = acc[21 + a];
        }
      }
    }
    __syncthreads();
  };

  // ---- max |x - Plus(x, -g)| over the free blocks, and |x|^2 over them
  auto gradient_max = [&]() -> double {
    double m = 0.0;
    if (tid < F) {
      if (hd->col[tid][0] >= 0) {
        const q4 q = q4{s_q[0][tid][0], s_q[0][tid][1], s_q[0][tid][2], s_q[0][tid][3]};
        const q4 p = sfmba_plus(q, mk3(-s_gc[tid][0], -s_gc[tid][1], -s_gc[tid][2]));
        m = fmax(fmax(fabs(q.w - p.w), fabs(q.x - p.x)), fmax(fabs(q.y - p.y), fabs(q.z - p.z)));
      }
      if (hd->col[tid][3] >= 0) m = fmax(m, fmax(fabs(s_gc[tid][3]), fmax(fabs(s_gc[tid][4]), fabs(s_gc[tid][5]))));
    }
    for (int i = tid; i < P; i += NT) {
      const double *g = pw + (size_t)i * SFMBA_PW + PW_G;
      m = fmax(m, fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))));
    }
    return block_max<NT>(m, red, tid);
  };
  auto x_norm_of = [&]() -> double {
    double s = 0.0;
    if (tid < F) {
      if (hd->col[tid][0] >= 0)
#pragma unroll
        for (int k = 0; k < 4; k++) s += s_q[0][tid][k] * s_q[0][tid][k];
      if (hd->col[tid][3] >= 0)
#pragma unroll
        for (int k = 0; k < 3; k++) s += s_t[0][tid][k] * s_t[0][tid][k];
    }
    for (int i = tid; i < P; i += NT) {
      const d3 x = ld3(X + 3 * (size_t)i);
      s += x.x * x.x + x.y * x.y + x.z * x.z;
    }
    return sqrt(block_sum<NT>(s, red, tid));
  };

  // ================= IterationZero
  double x_cost = evaluate(0, true);
  if (!isfinite(x_cost)) {
    if (tid == 0) res->nonfinite = 1;
    return;
  }
  camera_blocks();
  // jacobi_scaling: 1 / (1 + sqrt(squared column norm)), fixed here; zero on the constant columns
  if (tid < F) {
#pragma unroll
    for (int k = 0; k < 6; k++) s_sc[tid][k] = hd->col[tid][k] >= 0 ? 1.0 / (1.0 + sqrt(s_U[tid][7 * k])) : 0.0;
  }
  for (int i = tid; i < P; i += NT) {
    double *q = pw + (size_t)i * SFMBA_PW;
    q[PW_S] = 1.0 / (1.0 + sqrt(q[PW_V])), q[PW_S + 1] = 1.0 / (1.0 + sqrt(q[PW_V + 3])), q[PW_S + 2] = 1.0 / (1.0 + sqrt(q[PW_V + 5]));
  }
  __syncthreads();
  double x_norm = x_norm_of();
  double radius = 1e4, factor = 2.0;
  const double initial_cost = x_cost;
  int iteration = 0, n_succ = 0, n_unsucc = 0, n_invalid = 0, term = LFVIO_NO_CONVERGENCE, trace_len = 0;
  double it_cost = x_cost, it_change = 0.0, it_grad = gradient_max(), it_step = 0.0, it_rho = 0.0;
  int it_valid = 0, it_succ = 0;

  for (int pass = 0; pass <= LFVIO_MAX_TRACE; pass++) {  // every pass but a terminating one pushes an iteration: at most max_it + 1 <= LFVIO_MAX_TRACE
    // ---- FinalizeIterationAndCheckIfMinimizerCanContinue
    if (it_succ)
      n_succ++;
    else
      n_unsucc++;
    if (tid == 0 && trace_len < LFVIO_MAX_TRACE) {
      LfvioIterationSummary *d = &res->o.trace[trace_len];
      d->cost = it_cost, d->cost_change = it_change, d->gradient_max_norm = it_grad, d->step_norm = it_step, d->relative_decrease = it_rho;
      d->trust_region_radius = radius, d->step_is_valid = it_valid, d->step_is_successful = it_succ;
    }
    trace_len++;
    if (iteration >= max_it) {
      term = LFVIO_NO_CONVERGENCE;
      break;
    }
    if (it_succ && it_grad <= gtol) {
      term = LFVIO_CONVERGENCE;
      break;
    }
    if (radius <= 1e-32) {
      term = LFVIO_CONVERGENCE;
      break;
    }
    it_cost = x_cost, it_change = 0.0, it_grad = 0.0, it_step = 0.0, it_rho = 0.0, it_valid = 0, it_succ = 0;
    iteration++;

    // ---- LevenbergMarquardtStrategy::ComputeStep on the scaled Jacobian: D^2 = clamp(diag) / radius on every column
    for (int i = tid; i < P; i += NT) {
      double *q = pw + (size_t)i * SFMBA_PW;
      const double s0 = q[PW_S], s1 = q[PW_S + 1], s2 = q[PW_S + 2];
      double a = s0 * q[PW_V] * s0, b = s0 * q[PW_V + 1] * s1, c = s0 * q[PW_V + 2] * s2, d = s1 * q[PW_V + 3] * s1, e = s1 * q[PW_V + 4] * s2, f = s2 * q[PW_V + 5] * s2;
      a += sfmba_clamp(a) / radius, d += sfmba_clamp(d) / radius, f += sfmba_clamp(f) / radius;
      const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d, c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
      const double det = a * c00 + b * c01 + c * c02;
      const double Vi[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
      q[PW_VI] = Vi[0][0], q[PW_VI + 1] = Vi[0][1], q[PW_VI + 2] = Vi[0][2], q[PW_VI + 3] = Vi[1][1], q[PW_VI + 4] = Vi[1][2], q[PW_VI + 5] = Vi[2][2];
      const double sp[3] = {s0, s1, s2};
      q[PW_GS] = s0 * q[PW_G], q[PW_GS + 1] = s1 * q[PW_G + 1], q[PW_GS + 2] = s2 * q[PW_G + 2];
      for (int o = off[i]; o < off[i + 1]; o++) {
        double *w = ow + (size_t)o * SFMBA_OW;
        const double *sc = s_sc[frm[o]];
#pragma unroll
        for (int ca = 0; ca < 6; ca++) {
          double W[3];
#pragma unroll
          for (int cb = 0; cb < 3; cb++) {
            W[cb] = (sc[ca] * (w[OW_JC + ca] * w[OW_JP + cb] + w[OW_JC + 6 + ca] * w[OW_JP + 3 + cb] + w[OW_JC + 12 + ca] * w[OW_JP + 6 + cb])) * sp[cb];
            w[OW_W + 3 * ca + cb] = W[cb];
          }
#pragma unroll
          for (int cb = 0; cb < 3; cb++) w[OW_Y + 3 * ca + cb] = W[0] * Vi[0][cb] + W[1] * Vi[1][cb] + W[2] * Vi[2][cb];
        }
      }
    }
    __syncthreads();
    // the reduced system S = U + D^2 - sum W V^-1 W^T (lower triangle) and, as row n, the rhs -g_c + sum Y g_p
    for (int e = tid; e < (n + 1) * n; e += NT) {
      const int a = e / n, b = e - a * n;
      if (b > a) continue;
      const int fb = s_cf[b], cb = s_ck[b];
      double v;
      if (a < n) {
        const int fa = s_cf[a], ca = s_ck[a];
        v = 0.0;
        if (fa == fb) {
          v = s_sc[fa][ca] * s_U[fa][6 * ca + cb] * s_sc[fb][cb];
          if (a == b) v += sfmba_clamp(v) / radius;
        }
        // (no branch in the body: four points' loads are in flight at once; a point that lacks one of the frames reads observation 0 and adds nothing)
#pragma unroll 4
        for (int i = 0; i < P; i++) {
          const int oa = slot[(size_t)i * F + fa], ob = slot[(size_t)i * F + fb];
          const bool both = oa >= 0 && ob >= 0;
          const double *y = ow + (size_t)(both ? oa : 0) * SFMBA_OW + OW_Y + 3 * ca, *w = ow + (size_t)(both ? ob : 0) * SFMBA_OW + OW_W + 3 * cb;
          const double d = y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
          v -= both ? d : 0.0;
        }
      } else {
        v = -(s_sc[fb][cb] * s_gc[fb][cb]);
#pragma unroll 4
        for (int i = 0; i < P; i++) {
          const int ob = slot[(size_t)i * F + fb];
          const double *y = ow + (size_t)(ob >= 0 ? ob : 0) * SFMBA_OW + OW_Y + 3 * cb, *g = pw + (size_t)i * SFMBA_PW + PW_GS;
          const double d = y[0] * g[0] + y[1] * g[1] + y[2] * g[2];
          v += ob >= 0 ? d : 0.0;
        }
      }
      S[a * LD + b] = v;
    }
    // Cholesky, a column per step; row n (the rhs) rides along: L z = rhs.  A pivot that is not > 0 ends it (every thread reads the same pivot)
    bool bad = false;
    for (int k = 0; k < n; k++) {
      __syncthreads();
      const double d = S[k * LD + k];
      if (!(d > 0.0)) {
        bad = true;
        break;
      }
      const double l = sqrt(d);
      __syncthreads();
      for (int i = k + tid; i <= n; i += NT) S[i * LD + k] = i == k ? l : S[i * LD + k] / l;
      __syncthreads();
      const int m = n - k;  // rows k + 1 .. n, columns k + 1 .. n - 1
      for (int e = tid; e < m * (m - 1); e += NT) {
        const int i = k + 1 + e / (m - 1), j = k + 1 + e % (m - 1);
        if (j <= i) S[i * LD + j] -= S[i * LD + k] * S[j * LD + k];
      }
    }
    if (!bad) {  // L^T y = z
      for (int k = n - 1; k >= 0; k--) {
        __syncthreads();
        const double yk = S[n * LD + k] / S[k * LD + k];
        if (tid == 0) s_y[k] = yk;
        for (int j = tid; j < k; j += NT) S[n * LD + j] -= S[k * LD + j] * yk;
      }
    }
    __syncthreads();
    // the step: cameras delta = y scale; points y_p = V^-1 (-g_p - sum W^T y_c), delta = y_p scale
    double model_cost_change = 0.0;
    bool valid = false;
    if (!bad) {
      if (tid < F) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
          const int c = hd->col[tid][k];
          s_dc[tid][k] = c >= 0 ? s_y[c] : 0.0;  // y for now
        }
      }
      __syncthreads();
      double nonfinite = 0.0;
      for (int i = tid; i < P; i += NT) {
        double *q = pw + (size_t)i * SFMBA_PW;
        double h[3] = {-q[PW_GS], -q[PW_GS + 1], -q[PW_GS + 2]};
        for (int o = off[i]; o < off[i + 1]; o++) {
          const double *w = ow + (size_t)o * SFMBA_OW + OW_W, *y = s_dc[frm[o]];
#pragma unroll
          for (int cb = 0; cb < 3; cb++) h[cb] -= w[cb] * y[0] + w[3 + cb] * y[1] + w[6 + cb] * y[2] + w[9 + cb] * y[3] + w[12 + cb] * y[4] + w[15 + cb] * y[5];
        }
        const double *vi = q + PW_VI;
        const double d0 = (vi[0] * h[0] + vi[1] * h[1] + vi[2] * h[2]) * q[PW_S], d1 = (vi[1] * h[0] + vi[3] * h[1] + vi[4] * h[2]) * q[PW_S + 1],
                     d2 = (vi[2] * h[0] + vi[4] * h[1] + vi[5] * h[2]) * q[PW_S + 2];
        q[PW_D] = d0, q[PW_D + 1] = d1, q[PW_D + 2] = d2;
        if (!(isfinite(d0) && isfinite(d1) && isfinite(d2))) nonfinite = 1.0;
      }
      __syncthreads();
      if (tid < F) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
          s_dc[tid][k] *= s_sc[tid][k];
          if (!isfinite(s_dc[tid][k])) nonfinite = 1.0;
        }
      }
      nonfinite = block_max<NT>(nonfinite, red, tid);  // (its barriers also publish s_dc)
      if (nonfinite == 0.0) {
        // model_cost_change = -(J delta)^T (r + J delta / 2)
        double mc = 0.0;
        for (int i = tid; i < P; i += NT) {
          const double *dp = pw + (size_t)i * SFMBA_PW + PW_D;
          for (int o = off[i]; o < off[i + 1]; o++) {
            const double *w = ow + (size_t)o * SFMBA_OW, *dc = s_dc[frm[o]];
#pragma unroll
            for (int a = 0; a < 3; a++) {
              const double *jc = w + OW_JC + 6 * a, *jp = w + OW_JP + 3 * a;
              const double jd = (jc[0] * dc[0] + jc[1] * dc[1] + jc[2] * dc[2] + jc[3] * dc[3] + jc[4] * dc[4] + jc[5] * dc[5]) + (jp[0] * dp[0] + jp[1] * dp[1] + jp[2] * dp[2]);
              mc += jd * (w[OW_R + a] + 0.5 * jd);
            }
          }
        }
        model_cost_change = -block_sum<NT>(mc, red, tid);
        valid = model_cost_change > 0.0;
      }
    }
    it_valid = valid ? 1 : 0;
    if (!valid) {
      // HandleInvalidStep; LevenbergMarquardtStrategy::StepIsInvalid is StepRejected
      if (++n_invalid >= 5) {
        term = LFVIO_FAILURE;
        break;
      }
      radius = radius / factor, factor = 2.0 * factor;
      continue;
    }
    n_invalid = 0;
    // ---- the candidate x [+] delta, its cost, |x - candidate|
    double sn = 0.0;
    if (tid < F) {
      const q4 q = q4{s_q[0][tid][0], s_q[0][tid][1], s_q[0][tid][2], s_q[0][tid][3]};
      const q4 p = sfmba_plus(q, mk3(s_dc[tid][0], s_dc[tid][1], s_dc[tid][2]));
      s_q[1][tid][0] = p.w, s_q[1][tid][1] = p.x, s_q[1][tid][2] = p.y, s_q[1][tid][3] = p.z;
      const m33 R = sfmba_R(p);
#pragma unroll
      for (int k = 0; k < 9; k++) s_R[1][tid][k] = R.a[k];
#pragma unroll
      for (int k = 0; k < 3; k++) s_t[1][tid][k] = s_t[0][tid][k] + s_dc[tid][3 + k];
      if (hd->col[tid][0] >= 0) sn += (q.w - p.w) * (q.w - p.w) + (q.x - p.x) * (q.x - p.x) + (q.y - p.y) * (q.y - p.y) + (q.z - p.z) * (q.z - p.z);
      if (hd->col[tid][3] >= 0)
#pragma unroll
        for (int k = 0; k < 3; k++) sn += (s_t[0][tid][k] - s_t[1][tid][k]) * (s_t[0][tid][k] - s_t[1][tid][k]);
    }
    for (int i = tid; i < P; i += NT) {
      const double *dp = pw + (size_t)i * SFMBA_PW + PW_D;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double x = X[3 * (size_t)i + k], xc = x + dp[k];
        Xc[3 * (size_t)i + k] = xc;
        sn += (x - xc) * (x - xc);
      }
    }
    it_step = sqrt(block_sum<NT>(sn, red, tid));  // (its barriers also publish the candidate)
    double cand_cost = evaluate(1, false);
    if (!isfinite(cand_cost)) cand_cost = 1.79769313486231570815e+308;
    if (it_step <= ptol * (x_norm + ptol)) {
      term = LFVIO_CONVERGENCE;
      break;
    }
    it_change = x_cost - cand_cost;
    if (fabs(it_change) <= ftol * x_cost) {
      term = LFVIO_CONVERGENCE;
      break;
    }
    it_rho = it_change / model_cost_change;
    if (it_rho > 1e-3) {
      // HandleSuccessfulStep: x <- candidate, linearise there
      __syncthreads();
      if (tid < F) {
#pragma unroll
        for (int k = 0; k < 4; k++) s_q[0][tid][k] = s_q[1][tid][k];
#pragma unroll
        for (int k = 0; k < 3; k++) s_t[0][tid][k] = s_t[1][tid][k];
#pragma unroll
        for (int k = 0; k < 9; k++) s_R[0][tid][k] = s_R[1][tid][k];
      }
      for (int i = tid; i < P; i += NT)
#pragma unroll
        for (int k = 0; k < 3; k++) X[3 * (size_t)i + k] = Xc[3 * (size_t)i + k];
      __syncthreads();
      x_norm = x_norm_of();
      x_cost = evaluate(0, true);
      camera_blocks();
      it_cost = x_cost, it_grad = gradient_max(), it_succ = 1;
      const double u = 2.0 * it_rho - 1.0;
      radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - u * u * u));
      factor = 2.0;
    } else {
      // HandleUnsuccessfulStep / StepRejected
      it_cost = cand_cost;
      radius = radius / factor, factor = 2.0 * factor;
    }
  }

  // ---- the record: the state, Q = q.inverse(), T = -(Q * t) (initial_sfm.cpp:295-309)
  __syncthreads();
  if (tid < F) {
    const q4 q = q4{s_q[0][tid][0], s_q[0][tid][1], s_q[0][tid][2], s_q[0][tid][3]};
    const d3 t = mk3(s_t[0][tid][0], s_t[0][tid][1], s_t[0][tid][2]);
    qio[4 * tid] = q.w, qio[4 * tid + 1] = q.x, qio[4 * tid + 2] = q.y, qio[4 * tid + 3] = q.z;
    tio[3 * tid] = t.x, tio[3 * tid + 1] = t.y, tio[3 * tid + 2] = t.z;
    const double n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    const q4 Q = q4{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};  // Eigen's inverse(): conjugate / squared norm
    const d3 T = -qrot(Q, t);
    res->o.Q[tid][0] = Q.w, res->o.Q[tid][1] = Q.x, res->o.Q[tid][2] = Q.y, res->o.Q[tid][3] = Q.z;
    res->o.T[tid][0] = T.x, res->o.T[tid][1] = T.y, res->o.T[tid][2] = T.z;
  }
  if (tid == 0) {
    res->nonfinite = 0;
    res->o.termination = term, res->o.num_iterations = trace_len, res->o.num_successful_steps = n_succ, res->o.num_unsuccessful_steps = n_unsucc;
    res->o.initial_cost = initial_cost, res->o.final_cost = x_cost;
    res->o.accepted = (term == LFVIO_CONVERGENCE || x_cost < 5e-3) ? 1 : 0;
  }
}
