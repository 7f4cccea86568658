// kernels_twoview.h — the two-view RANSAC behind ESTIMATE_EXTRINSIC == 2 (initial/initial_ex_rotation.cpp:69-368).
//
//   k_tv_hyp : compute_E_21 on an 8-match sample + check_inliers over all matches          :69-155, :180-196
//              grid S x 64, one wave per hypothesis
//   k_tv_fit : selection (:197-202), refit over the winner's inliers (:204-218), decomposeE (:321-336),
//              testTriangulation of the four candidates (:289-319, :338-353), the choice of solveRelativeR (:276-284)
//              one workgroup of 256
//
// The essential matrix is estimated on bearing vectors, so rays with z <= 0 are ordinary inputs.  Null vectors come from
// Householder factorizations of the systems themselves (never of A^T A): of the 9 x 8 transpose for a sample, whose last
// column of Q is the null vector; of the n x 9 inlier system down to a 9 x 9 triangle for the refit, whose smallest right
// singular vector the wave-wide Jacobi from dev_smallmat.h finds.  Rows of matches that are not inliers enter the refit as
// zero rows: they add exact zeros to every sum, so the triangle is the one of the compacted system and no inlier list is
// needed.
// The score is the reference's: a FLOAT accumulator taking double terms match by match, in match order, against the FLOAT
// threshold — one lane walks the terms the others left in LDS.
// The bodies are device functions (tv_hyp_body, tv_fit_body): solve_5pts.cpp restates the same steps for relativePose(), and
// kernels_relpose.h runs them per candidate pair.
#pragma once
#include "dev_smallmat.h"

constexpr int TV_HYP_THREADS = 64, TV_FIT_THREADS = 256, TV_CHUNK = 1024;
constexpr int TV_MAX_MATCHES = 4096, TV_MAX_SAMPLES = 1024;
constexpr float TV_RESIDUAL_COS_THR = 0.00872653549837f;  // :109

// Unit null vector of the 8 x 9 system whose transpose is M (9 x 8): Householder QR of M, v = Q e_8.  Thread-private and
// fully unrolled (every index is a compile-time constant).  A column that is already zero below its diagonal gets the
// identity for a reflector, so a degenerate sample gives finite numbers.
DEV void tv_null9(double (&M)[9][8], double (&v)[9]) {
  double beta[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    double s = 0;
#pragma unroll
    for (int r = k; r < 9; r++) s += M[r][k] * M[r][k];
    const double nrm = sqrt(s), alpha = M[k][k] > 0 ? -nrm : nrm;
    M[k][k] -= alpha;  // rows k .. 8 of column k now hold the reflector's vector
    double vtv = 0;
#pragma unroll
    for (int r = k; r < 9; r++) vtv += M[r][k] * M[r][k];
    beta[k] = vtv > 0 ? 2.0 / vtv : 0.0;
#pragma unroll
    for (int c = k + 1; c < 8; c++) {
      double d = 0;
#pragma unroll
      for (int r = k; r < 9; r++) d += M[r][k] * M[r][c];
      d *= beta[k];
#pragma unroll
      for (int r = k; r < 9; r++) M[r][c] -= d * M[r][k];
    }
  }
#pragma unroll
  for (int r = 0; r < 9; r++) v[r] = r == 8 ? 1.0 : 0.0;
#pragma unroll
  for (int k = 7; k >= 0; k--) {
    double d = 0;
#pragma unroll
    for (int r = k; r < 9; r++) d += M[r][k] * v[r];
    d *= beta[k];
#pragma unroll
    for (int r = k; r < 9; r++) v[r] -= d * M[r][k];
  }
}

// E_0 = v read as a row-major 3 x 3; its SVD as B = E_0 V (columns of B: sigma_c u_c), columns sorted by falling norm;
// E = E_0 with the smallest singular value dropped (:89-97).  B, V and the squared column norms are returned for
// decomposeE.
DEV void tv_rank2(const double (&v)[9], double (&E)[9], double (&B)[3][3], double (&V)[3][3], double (&n2)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) B[i][j] = v[3 * i + j];
  svd3_sorted(B, V, n2);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) E[3 * i + j] = B[i][0] * V[j][0] + B[i][1] * V[j][1];
}

// check_inliers for one match (:111-151).  c2 / c1: the score terms (thr - residual)^2 of frame 2 and frame 1, -1 where the
// residual exceeds the threshold (a NaN residual passes, as `thr < NaN` is false in the reference too); c1 is only
// meaningful when c2 passed.  Returns whether the match is an inlier.
DEV bool tv_residual(const double (&E)[9], d3 bl, d3 br, double &c2, double &c1) {
  const double thr = (double)TV_RESIDUAL_COS_THR;
  const d3 e2 = mk3(E[0] * bl.x + E[1] * bl.y + E[2] * bl.z, E[3] * bl.x + E[4] * bl.y + E[5] * bl.z, E[6] * bl.x + E[7] * bl.y + E[8] * bl.z);
  const double r2 = fabs((e2.x * br.x + e2.y * br.y + e2.z * br.z) / sqrt(e2.x * e2.x + e2.y * e2.y + e2.z * e2.z));
  c1 = -1.0;
  if (thr < r2) {
    c2 = -1.0;
    return false;
  }
  c2 = (thr - r2) * (thr - r2);
  const d3 e1 = mk3(E[0] * br.x + E[3] * br.y + E[6] * br.z, E[1] * br.x + E[4] * br.y + E[7] * br.z, E[2] * br.x + E[5] * br.y + E[8] * br.z);
  const double r1 = fabs((e1.x * bl.x + e1.y * bl.y + e1.z * bl.z) / sqrt(e1.x * e1.x + e1.y * e1.y + e1.z * e1.z));
  if (thr < r1) return false;
  c1 = (thr - r1) * (thr - r1);
  return true;
}

// Hypothesis on the matches idx8[0 .. 8) of bl / br [N][3]: E to E_out[9], the score to *score_out.  One wave; s2 / s1: TV_CHUNK
// doubles of LDS each.  Every lane runs the same 8-point solve (a wave issues it once either way); the residuals are
// lanes-parallel, a chunk of matches at a time.  Shared by k_tv_hyp and k_rp_hyp (kernels_relpose.h).
DEV void tv_hyp_body(int N, const double *bl, const double *br, const int *idx8, double *E_out, float *score_out, double *s2, double *s1, int lane) {
  int idx[8];
#pragma unroll
  for (int j = 0; j < 8; j++) idx[j] = idx8[j];
  d3 pl[8], pr[8];
#pragma unroll
  for (int j = 0; j < 8; j++) pl[j] = ld3(bl + 3 * (size_t)idx[j]), pr[j] = ld3(br + 3 * (size_t)idx[j]);
  double M[9][8], v[9], E[9], B[3][3], V[3][3], n2[3];
#pragma unroll
  for (int j = 0; j < 8; j++) {  // :78-80, transposed
    M[0][j] = pr[j].x * pl[j].x, M[1][j] = pr[j].x * pl[j].y, M[2][j] = pr[j].x * pl[j].z;
    M[3][j] = pr[j].y * pl[j].x, M[4][j] = pr[j].y * pl[j].y, M[5][j] = pr[j].y * pl[j].z;
    M[6][j] = pr[j].z * pl[j].x, M[7][j] = pr[j].z * pl[j].y, M[8][j] = pr[j].z * pl[j].z;
  }
  tv_null9(M, v);
  tv_rank2(v, E, B, V, n2);
  if (lane < 9) {
    double e = E[0];
#pragma unroll
    for (int j = 1; j < 9; j++) e = lane == j ? E[j] : e;
    E_out[lane] = e;
  }
  float score = 0.0f;
  for (int base = 0; base < N; base += TV_CHUNK) {
    const int end = min(N, base + TV_CHUNK);
    for (int i = base + lane; i < end; i += TV_HYP_THREADS) {
      double c2, c1;
      tv_residual(E, ld3(bl + 3 * (size_t)i), ld3(br + 3 * (size_t)i), c2, c1);
      s2[i - base] = c2, s1[i - base] = c1;
    }
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < end - base; i++) {
        const double c2 = s2[i], c1 = s1[i];
        if (!(c2 < 0.0)) {
          score = (float)((double)score + c2);  // :132
          if (!(c1 < 0.0)) score = (float)((double)score + c1);  // :150
        }
      }
    __syncthreads();
  }
  if (lane == 0) *score_out = score;
}

// grid S x 64: hypothesis k on the matches samples[8 k .. 8 k + 8).
__global__ __launch_bounds__(TV_HYP_THREADS) void k_tv_hyp(int N, const double *bl, const double *br, const int *samples, double *E_all,
                                                           float *score_all) {
  __shared__ double s2[TV_CHUNK], s1[TV_CHUNK];
  const int k = blockIdx.x;
  tv_hyp_body(N, bl, br, samples + 8 * (size_t)k, E_all + 9 * (size_t)k, score_all + k, s2, s1, threadIdx.x);
}

// Step K of the Householder QR of A (NR x 9, rows striped over the NT threads): column K below the diagonal to zero.
template <int NT, int K>
DEV void tv_qr_step(double *A, int NR, double *red, int tid) {
  __syncthreads();  // the stores of the step before
  double s = 0;
  for (int i = tid; i < NR; i += NT)
    if (i >= K) {
      const double x = A[9 * (size_t)i + K];
      s += x * x;
    }
  s = block_sum<NT>(s, red, tid);
  const double xk = A[9 * (size_t)K + K], nrm = sqrt(s), alpha = xk > 0 ? -nrm : nrm, vk = xk - alpha;
  const double vtv = (s - xk * xk) + vk * vk, beta = vtv > 0 ? 2.0 / vtv : 0.0;
  if constexpr (K < 8) {
    double d[8 - K];
#pragma unroll
    for (int c = 0; c < 8 - K; c++) d[c] = 0;
    for (int i = tid; i < NR; i += NT)
      if (i >= K) {
        const double *a = A + 9 * (size_t)i;
        const double vi = i == K ? vk : a[K];
#pragma unroll
        for (int c = 0; c < 8 - K; c++) d[c] += vi * a[K + 1 + c];
      }
    block_sum_n<NT, 8 - K>(d, red, tid);
    for (int i = tid; i < NR; i += NT)
      if (i >= K) {
        double *a = A + 9 * (size_t)i;
        const double vi = i == K ? vk : a[K];
#pragma unroll
        for (int c = 0; c < 8 - K; c++) a[K + 1 + c] -= (beta * d[c]) * vi;
      }
  }
  if (tid == K % NT) A[9 * (size_t)K + K] = alpha;
}

// The LDS of tv_fit_body, and what it leaves in every thread's registers.
struct TvFitLds {
  float sc[TV_MAX_SAMPLES];
  double red[8 * TV_FIT_THREADS / 64], sv[9];
  int sbest, cnt[4];  // cnt: the four candidates' counts in testTriangulation's order (R1,t) (R1,-t) (R2,t) (R2,-t)
};
struct TvFit {
  int best, n_in;  // the winning hypothesis (-1: none scored > 0); its inliers before the refit (status 1) or after it (status 0)
  double best_score, E[9];
  m33 R1, R2;
  d3 u3;
};

// One workgroup of TV_FIT_THREADS: selection, refit, mask, decomposition and the 4 x N triangulations.  A: scratch of max(N, 9) x 9
// doubles.  Returns lfvio_two_view's status, the same in every thread; with 0 the mask and lds.cnt are written and f is complete,
// with 1 only f.best, f.n_in and f.best_score are.  UNIT: a match counts when both dot products DIVIDED BY THE NORMS of the
// triangulated point are > 0 (recoverPose, solve_5pts.cpp:436-440: a non-finite point does not count) instead of the plain dot
// products of testTriangulation (initial_ex_rotation.cpp:310-311).  Shared by k_tv_fit and k_rp_fit (kernels_relpose.h).
// MASK_ONLY: stop behind the returned mask (k_trk_fit, kernels_track.h: rejectWithF keeps nothing else); with 0 the mask, f.best,
// f.n_in, f.best_score and f.E are written and nothing more.
template <bool UNIT, bool MASK_ONLY = false>
DEV int tv_fit_body(int N, int S, const double *bl, const double *br, const double *E_all, const float *score_all, double *A, unsigned char *mask,
                    TvFitLds &lds, TvFit &f) {
  constexpr int NT = TV_FIT_THREADS;
  float *sc = lds.sc;
  double *red = lds.red, *sv = lds.sv;
  int &sbest = lds.sbest, *cnt = lds.cnt;
  const int tid = threadIdx.x, NR = max(N, 9);
  for (int k = tid; k < S; k += NT) sc[k] = score_all[k];
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  if (tid == 0) {  // :169-170, :197-202: strict <, the first of equal scores wins
    double best_score = 0.0;
    int b = -1;
    for (int k = 0; k < S; k++)
      if (best_score < (double)sc[k]) best_score = (double)sc[k], b = k;
    sbest = b;
  }
  __syncthreads();
  const int best = sbest;
  f.best = best, f.n_in = 0, f.best_score = 0.0;
  if (best < 0) return 1;
  f.best_score = (double)sc[best];
  double (&E)[9] = f.E;
#pragma unroll
  for (int j = 0; j < 9; j++) E[j] = E_all[9 * (size_t)best + j];
  // the winner's inliers (the same arithmetic on the same bits as in k_tv_hyp) and the rows of the refit system
  double n_in = 0;
  for (int i = tid; i < NR; i += NT) {
    bool in = false;
    d3 l = mk3(0, 0, 0), r = mk3(0, 0, 0);
    if (i < N) {
      double c2, c1;
      l = ld3(bl + 3 * (size_t)i), r = ld3(br + 3 * (size_t)i);
      in = tv_residual(E, l, r, c2, c1);
    }
    const double w = in ? 1.0 : 0.0;
    n_in += w;
    double *a = A + 9 * (size_t)i;
    a[0] = w * (r.x * l.x), a[1] = w * (r.x * l.y), a[2] = w * (r.x * l.z);
    a[3] = w * (r.y * l.x), a[4] = w * (r.y * l.y), a[5] = w * (r.y * l.z);
    a[6] = w * (r.z * l.x), a[7] = w * (r.z * l.y), a[8] = w * (r.z * l.z);
  }
  n_in = block_sum<NT>(n_in, red, tid);
  f.n_in = (int)n_in;
  if (n_in < 8.0) return 1;
  // Householder QR of A down to a 9 x 9 triangle
  tv_qr_step<NT, 0>(A, NR, red, tid), tv_qr_step<NT, 1>(A, NR, red, tid), tv_qr_step<NT, 2>(A, NR, red, tid);
  tv_qr_step<NT, 3>(A, NR, red, tid), tv_qr_step<NT, 4>(A, NR, red, tid), tv_qr_step<NT, 5>(A, NR, red, tid);
  tv_qr_step<NT, 6>(A, NR, red, tid), tv_qr_step<NT, 7>(A, NR, red, tid), tv_qr_step<NT, 8>(A, NR, red, tid);
  __syncthreads();
  // smallest right singular vector of the triangle, in wave 0: lane r holds row r of R and of V
  if (tid < 64) {
    double G[9], W[9], g2[9];
#pragma unroll
    for (int c = 0; c < 9; c++) G[c] = (tid < 9 && c >= tid) ? A[9 * (size_t)min(tid, 8) + c] : 0.0;
    jacobi_wave<9>(G, W, g2, tid);
    double bn = 0, vv = 0;
#pragma unroll
    for (int c = 0; c < 9; c++)
      if (c == 0 || g2[c] < bn) bn = g2[c], vv = W[c];
    if (tid < 9) sv[tid] = vv;
  }
  __syncthreads();
  double v[9], B[3][3], V[3][3], n2[3];
#pragma unroll
  for (int j = 0; j < 9; j++) v[j] = sv[j];
  tv_rank2(v, E, B, V, n2);
  // check_inliers of the refit: the mask that is returned (:217)
  n_in = 0;
  for (int i = tid; i < N; i += NT) {
    double c2, c1;
    const bool in = tv_residual(E, ld3(bl + 3 * (size_t)i), ld3(br + 3 * (size_t)i), c2, c1);
    mask[i] = in ? 1 : 0;
    n_in += in ? 1.0 : 0.0;
  }
  n_in = block_sum<NT>(n_in, red, tid);
  f.n_in = (int)n_in;
  if constexpr (MASK_ONLY) return 0;
  // decomposeE (:321-336) from the SVD the projection already holds: E = sigma_1 u_1 v_1^T + sigma_2 u_2 v_2^T.  u_3 and
  // v_3 are the cross products, so det U = det V = +1 and both candidates are proper rotations.
  d3 u1, u2, u3;
  svd3_u(B, n2, u1, u2, u3);
  const d3 v1 = mk3(V[0][0], V[1][0], V[2][0]), v2 = mk3(V[0][1], V[1][1], V[2][1]), v3 = cross(v1, v2);
  const double U1[3] = {u1.x, u1.y, u1.z}, U2[3] = {u2.x, u2.y, u2.z}, U3[3] = {u3.x, u3.y, u3.z};
  const double V1[3] = {v1.x, v1.y, v1.z}, V2[3] = {v2.x, v2.y, v2.z}, V3[3] = {v3.x, v3.y, v3.z};
  m33 &R1 = f.R1, &R2 = f.R2;  // U W V^T and U W^T V^T
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double a = U2[i] * V1[j] - U1[i] * V2[j], b = U3[i] * V3[j];
      R1.a[3 * i + j] = a + b, R2.a[3 * i + j] = b - a;
    }
  // testTriangulation: this thread's candidate is fixed (NT is a multiple of 4), its matches are tid / 4 + k NT / 4
  {
    const int cand = tid & 3;
    m33 R;  // (element by element: a select between the two structs would go through memory)
#pragma unroll
    for (int j = 0; j < 9; j++) R.a[j] = cand < 2 ? R1.a[j] : R2.a[j];
    const d3 t = (cand & 1) ? -u3 : u3;
    int front = 0;
    for (int i = tid >> 2; i < N; i += NT / 4) {
      const d3 l = ld3(bl + 3 * (size_t)i), r = ld3(br + 3 * (size_t)i);
      double D[4][4], Q[4][4];
      D[0][0] = -l.z, D[0][1] = 0.0, D[0][2] = l.x, D[0][3] = 0.0;  // :343-344 with Pose0 = [I | 0]
      D[1][0] = 0.0, D[1][1] = -l.z, D[1][2] = l.y, D[1][3] = 0.0;
      const double P0[4] = {R.a[0], R.a[1], R.a[2], t.x}, P1[4] = {R.a[3], R.a[4], R.a[5], t.y}, P2[4] = {R.a[6], R.a[7], R.a[8], t.z};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        D[2][c] = r.x * P2[c] - r.z * P0[c];  // :345
        D[3][c] = r.y * P2[c] - r.z * P1[c];  // :346
      }
      jacobi_cols<4, 4>(D, Q, 2.3e-16);
      double q0 = 0, q1 = 0, q2 = 0, q3 = 0, bn = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const double m2 = D[0][c] * D[0][c] + D[1][c] * D[1][c] + D[2][c] * D[2][c] + D[3][c] * D[3][c];
        if (c == 0 || m2 < bn) bn = m2, q0 = Q[0][c], q1 = Q[1][c], q2 = Q[2][c], q3 = Q[3][c];
      }
      const d3 X = mk3(q0 / q3, q1 / q3, q2 / q3);  // :350-352
      const d3 Xr = mk3(R.a[0] * X.x + R.a[1] * X.y + R.a[2] * X.z + t.x, R.a[3] * X.x + R.a[4] * X.y + R.a[5] * X.z + t.y,
                        R.a[6] * X.x + R.a[7] * X.y + R.a[8] * X.z + t.z);
      const double dl = l.x * X.x + l.y * X.y + l.z * X.z, dr = r.x * Xr.x + r.y * Xr.y + r.z * Xr.z;  // :310-311
      if constexpr (UNIT) {
        const double nl = sqrt(X.x * X.x + X.y * X.y + X.z * X.z), nr = sqrt(Xr.x * Xr.x + Xr.y * Xr.y + Xr.z * Xr.z);
        if (dl / nl > 0 && dr / nr > 0) front++;
      } else {
        if (dl > 0 && dr > 0) front++;
      }
    }
    atomicAdd(&cnt[cand], front);  // integers: the order does not matter
  }
  __syncthreads();
  f.u3 = u3;
  return 0;
}

// One workgroup.  out is written on every path; mask only when status == 0.
__global__ __launch_bounds__(TV_FIT_THREADS) void k_tv_fit(int N, int S, const double *bl, const double *br, const double *E_all,
                                                           const float *score_all, double *A, unsigned char *mask, LfvioTwoViewOut *out) {
  __shared__ TvFitLds lds;
  TvFit f;
  const int status = tv_fit_body<false>(N, S, bl, br, E_all, score_all, A, mask, lds, f);
  if (threadIdx.x != 0) return;
  out->status = status, out->best_sample = f.best, out->num_inliers = f.n_in, out->best_score = f.best_score;
  if (status == 0) {
    double fr[4];
#pragma unroll
    for (int j = 0; j < 9; j++) out->E[j] = f.E[j], out->R_cand[0][j] = f.R1.a[j], out->R_cand[1][j] = f.R2.a[j];
    out->t_cand[0] = f.u3.x, out->t_cand[1] = f.u3.y, out->t_cand[2] = f.u3.z;
#pragma unroll
    for (int j = 0; j < 4; j++) fr[j] = 1.0 * lds.cnt[j] / N, out->front[j] = fr[j];
    const double ratio1 = fmax(fr[0], fr[1]), ratio2 = fmax(fr[2], fr[3]);  // :276-278
    const bool first = ratio1 > ratio2;                                     // :280-284: transposed
#pragma unroll
    for (int j = 0; j < 9; j++) out->R_rel[j] = first ? f.R1.a[3 * (j % 3) + j / 3] : f.R2.a[3 * (j % 3) + j / 3];
  }
}
