// kernels_relpose.h — Estimator::relativePose() (estimator.cpp:445-473) over MotionEstimator::solveRelativeRT
// (initial/solve_5pts.cpp:201-576) for every candidate pair of the window in one call.
//
//   k_rp_hyp : grid (S + 1, P) x 64.  Block (x < S, p): hypothesis x of pair p — tv_hyp_body on the pair's slice of the matches
//              (compute_E_21 :201-230, check_inliers :231-273); returns at once where N_p <= 20 (estimator.cpp:452).
//              Block (S, p): the pair's parallax (:454-463) and its gate word, so the sequential sum is off the chain of k_rp_fit.
//   k_rp_fit : grid P x 256.  Returns at once for a gated pair; otherwise tv_fit_body (myfindFundamentalMat's selection and refit
//              :311-334, decomposeEssentialMat :337-362, the 4 x N triangulations :364-394), then recoverPose's counts in ITS order
//              (:430-501), its choice (:507-534), the verdict (:570) and the intended output (include/lfvio.h, deviation 1).
//
// The arithmetic of solve_5pts.cpp is the arithmetic of initial_ex_rotation.cpp: the bodies are the device functions of
// kernels_twoview.h, not copies.  The parallax terms are computed lanes-parallel into LDS, TV_CHUNK at a time, and ONE lane adds them
// in match order, as the float score is added.
#pragma once
#include "kernels_twoview.h"

constexpr int RP_MIN_MATCHES = 20;  // a pair runs when N > 20 (estimator.cpp:452)

// rows of the refit scratch in front of pair p: every pair takes max(N_p, 9) <= N_p + 9 rows
DEV size_t rp_scratch_row(const int *off, int p) { return (size_t)off[p] + 9 * (size_t)p; }

__global__ __launch_bounds__(TV_HYP_THREADS) void k_rp_hyp(int S, const int *off, const double *bl, const double *br, const int *samples,
                                                           double *E_all, float *score_all, int *gate, LfvioRelativePosePair *rec) {
  __shared__ double s2[TV_CHUNK], s1[TV_CHUNK];
  const int x = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
  const int o = off[p], N = off[p + 1] - o;
  bl += 3 * (size_t)o, br += 3 * (size_t)o;
  if (x < S) {
    if (N <= RP_MIN_MATCHES) return;
    const size_t k = (size_t)p * S + x;
    tv_hyp_body(N, bl, br, samples + 8 * k, E_all + 9 * k, score_all + k, s2, s1, lane);
    return;
  }
  if (N <= RP_MIN_MATCHES) {
    if (lane == 0) gate[p] = 1, rec[p].gate = 1, rec[p].num_matches = N;
    return;
  }
  double sum = 0.0;
  for (int base = 0; base < N; base += TV_CHUNK) {
    const int end = min(N, base + TV_CHUNK);
    for (int i = base + lane; i < end; i += TV_HYP_THREADS) {
      const d3 l = ld3(bl + 3 * (size_t)i), r = ld3(br + 3 * (size_t)i);
      const double dx = l.x / l.z - r.x / r.z, dy = l.y / l.z - r.y / r.z;  // :458-459 (z == 0: inf / NaN, kept)
      s2[i - base] = sqrt(dx * dx + dy * dy);                               // :460
    }
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < end - base; i++) sum = sum + s2[i];  // :461
    __syncthreads();
  }
  if (lane == 0) {
    const double avg = 1.0 * sum / N;             // :463
    const int g = avg * 160 > 30 ? 0 : 2;         // :464 (NaN > 30 is false)
    gate[p] = g, rec[p].gate = g, rec[p].num_matches = N, rec[p].average_parallax = avg;
  }
}

__global__ __launch_bounds__(TV_FIT_THREADS) void k_rp_fit(int S, const int *off, const double *bl, const double *br, const double *E_all,
                                                           const float *score_all, const int *gate, double *A, unsigned char *mask,
                                                           LfvioRelativePosePair *rec) {
  __shared__ TvFitLds lds;
  const int p = blockIdx.x;
  if (gate[p] != 0) return;
  const int o = off[p], N = off[p + 1] - o;
  TvFit f;
  const int status = tv_fit_body<true>(N, S, bl + 3 * (size_t)o, br + 3 * (size_t)o, E_all + 9 * (size_t)p * S, score_all + (size_t)p * S,
                                       A + 9 * rp_scratch_row(off, p), mask + o, lds, f);
  if (threadIdx.x != 0) return;
  LfvioRelativePosePair *out = rec + p;
  out->best_sample = f.best, out->num_inliers = f.n_in, out->best_score = f.best_score;
  if (status != 0) {
    out->gate = 3;
    return;
  }
#pragma unroll
  for (int j = 0; j < 9; j++) out->E[j] = f.E[j], out->R_cand[0][j] = f.R1.a[j], out->R_cand[1][j] = f.R2.a[j];
  out->t_cand[0] = f.u3.x, out->t_cand[1] = f.u3.y, out->t_cand[2] = f.u3.z;
  const int g1 = lds.cnt[0], g2 = lds.cnt[2], g3 = lds.cnt[1], g4 = lds.cnt[3];  // (R1,t) (R2,t) (R1,-t) (R2,-t)
  out->good[0] = g1, out->good[1] = g2, out->good[2] = g3, out->good[3] = g4;
  int chosen, cnt;  // :507-534
  if (g1 >= g2 && g1 >= g3 && g1 >= g4)
    chosen = 0, cnt = g1;
  else if (g2 >= g1 && g2 >= g3 && g2 >= g4)
    chosen = 1, cnt = g2;
  else if (g3 >= g1 && g3 >= g2 && g3 >= g4)
    chosen = 2, cnt = g3;
  else
    chosen = 3, cnt = g4;
  out->chosen = chosen, out->inlier_cnt = cnt, out->ok = cnt > 12 ? 1 : 0;  // :570
  const bool second = (chosen & 1) != 0, neg = chosen >= 2;
  double R[9];
#pragma unroll
  for (int j = 0; j < 9; j++) R[j] = second ? f.R2.a[j] : f.R1.a[j];
  const double t[3] = {neg ? -f.u3.x : f.u3.x, neg ? -f.u3.y : f.u3.y, neg ? -f.u3.z : f.u3.z};
#pragma unroll
  for (int j = 0; j < 9; j++) out->rot[j] = R[j], out->rotation[j] = R[3 * (j % 3) + j / 3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    out->trans[i] = t[i];
    out->translation[i] = (-R[i]) * t[0] + (-R[3 + i]) * t[1] + (-R[6 + i]) * t[2];  // -R^T t
  }
}
