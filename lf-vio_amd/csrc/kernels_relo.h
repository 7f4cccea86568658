// kernels_relo.h — the relocalization route of Estimator::optimization() (estimator.cpp:777-808, lfvio_solve_relo).
//
// A loop-closure message adds one parameter block, relo_Pose (7 global / 6 local, PoseLocalParameterization), and one plain
// ProjectionFactor per matched landmark on (para_Pose[start_frame], relo_Pose, para_Ex_Pose, para_Feature[l])
// (factor/projection_factor.cpp:21-121: no td column even when ESTIMATE_TD is on).  The reduced camera system grows from
// KP = 172 to RK = 178: the existing ordering with the relo tangent appended.  Landmarks stay one-dimensional, so their
// elimination is still a sum of rank-1 terms w_l w_l^T / h_l; a landmark with a relo factor has six more non-zeros in w_l.
//
// This route is separate from the resident ones (k_lin / k_linw / k_linb + k_solve_dense): a relo solve happens once per
// loop-closure message, not per frame, so it is laid out for clarity and a bounded size rather than for the last microsecond:
//   k_relo_setup    IMU sqrt_info (LLT of the inverse covariance), state and trust-region header (tr_init, as k_setup)
//   k_relo_eval     one lane per landmark: its visual factors + its relo factor, Cauchy-corrected; the camera-side Jacobian
//                   rows go to a dense row table [178 columns | r], the landmark column straight into w_l, h_l, g_l, cost.
//                   Behind the landmark workgroups: one workgroup per IMU factor and one for the prior.  Cost-only form for
//                   the candidate of a pass.
//   k_relo_gram     H_cc | g_c = rows^T rows, 16 x 16 output tiles x row chunks, fixed summation order (no atomics)
//   k_relo_schur    the Schur complement of the landmark block + mu diagonal and the reduced rhs, 16 x 16 tiles
//   k_relo_solve    one workgroup; phase 0 (a new linearization): Jacobi scaling (Ceres' 1 / (1 + |J_col|), fixed at the start point), the D diagonal, the
//                   gradient max-norm, Cauchy-point terms; phase 1: packed Cholesky of the reduced system in LDS (retries with a
//                   raised mu form it there), back-substitution,
//                   the dogleg and the candidate x (+) delta
//   k_relo_decide   TrustRegionMinimizer's accept / reject / terminate policy: decide_walk of tr_decide.h, one candidate per pass
// The loop header is the resident routes' TRState; the workgroup reductions are dev_math.h's.
// Semantics: tests/relo_ref.py, a numpy statement of the same Ceres 1.12 loop over the augmented state.
#pragma once
#include "dev_factors.h"
#include "tr_decide.h"

constexpr int RK = KP + 6;     // reduced system: 172 + relo tangent
constexpr int RO = KP;         // first column of the relo tangent
constexpr int RLD = RK + 2;    // a Jacobian row: [178 camera-side columns | corrected residual | pad]
constexpr int RG = RK + 1;     // gram output: (RK + 1) x (RK + 1), column RK = J^T r
constexpr int RELO_MAX_LM = 2048;  // landmarks of a relo window (lfvio_solve_relo refuses more: LFVIO_ERR_ARG)
constexpr int RELO_LM_WG = 64;     // landmarks per workgroup of k_relo_eval
constexpr int RELO_GCH = 8;        // row chunks of k_relo_gram
constexpr int RELO_GT = (RG + 15) / 16;                 // 12 tile rows
constexpr int RELO_GTILES = RELO_GT * (RELO_GT + 1) / 2;  // 78 upper tiles
constexpr int RELO_STILES = RELO_GTILES + 1;               // k_relo_schur: the lower tiles of S, then one workgroup for the rhs
constexpr int RELO_SOLVE_THREADS = 1024;
constexpr int RPACK = RK * (RK + 1) / 2;  // packed lower triangle of the reduced system
constexpr size_t RELO_SOLVE_LDS = (size_t)(RPACK + RK + RELO_MAX_LM + 64) * sizeof(double);
constexpr int RELO_PCOST = LFVIO_WINDOW_SIZE + 1;  // pose-side cost items: IMU factors, prior

struct ReloX {  // one point of the augmented state
  FrameState f;
  double relo[7];
};

struct ReloDev {
  int N, M, K, R, est_ex, est_td, relo_on, prior_n, prior_nb, max_iter;
  int row_relo, row_imu, row_prior;
  double sqrt_info, tr_ro, row, g[3];  // tr_ro: TR, the rolling-shutter read-out time
  // inputs
  const int *start, *off, *rk;  // rk[l]: the landmark's match, -1: none
  const double *pt, *vel, *ctd, *uvy, *mp, *lam0;
  LfvioPreintegration imu[LFVIO_WINDOW_SIZE];
  int imu_on[LFVIO_WINDOW_SIZE];
  double imu_sqrt[LFVIO_WINDOW_SIZE][225];
  int prior_kind[LFVIO_MAX_PRIOR_BLOCKS], prior_frame[LFVIO_MAX_PRIOR_BLOCKS], prior_idx[LFVIO_MAX_PRIOR_BLOCKS];
  double prior_x0[LFVIO_MAX_PRIOR_BLOCKS][9];
  const double *prior_J, *prior_r;
  ReloX x0;
  // state: x[cur] is the current point, x[cur ^ 1] the candidate
  ReloX x[2];
  double *lam[2];
  // work arrays
  double *J;       // [R][RLD]
  double *gpart;   // [RELO_GCH][RG][RG]
  double *Hs;      // [RK][RK] scaled camera-side Hessian
  double *Sg;      // [RK][RK + 1] Schur complement + mu D^2 | reduced rhs, at mu = Sg_mu (k_relo_schur)
  double Sg_mu;
  double *gs;      // [RK] scaled gradient
  double *W;       // [N][RK] w_l (unscaled after k_relo_eval, scaled by k_relo_solve)
  double *h, *gl;  // [N]
  double *lcost;   // [N]
  double pcost[RELO_PCOST];
  double scale[RK], diag[RK], gn[RK], stp[RK];
  double *scale_l, *diag_l, *gn_l, *stp_l, *hs, *gsl;  // [N]
  int act[RK];
  double mlin, mquad;  // the candidate's model terms s.g and s^T H s (k_relo_solve; decide_walk's DecideSums)
  // the loop header.  Only a part of it is used: one candidate per pass (cg = cn = 0 and q[] = 0, the whole step is in mlin / mquad);
  // step_sq_pose, xn2_pose_cand: |delta|^2 and |x (+) delta|^2 of the whole augmented state; scaled: IterationZero is behind
  TRState tr;
};

// ProjectionTdFactor / ProjectionFactor::Evaluate (projection_td_factor.cpp:36-151, projection_factor.cpp:21-121), one
// factor in the literal form of tests/np_ref.py::visual: the residual chain rotates back with Quaternion::inverse(), the
// Jacobians with the transposed rotation matrices.  Outputs: r[2], Ji / Jj / Jex [2][6], Jl[2], Jtd[2].
DEV void relo_visual(bool use_td, double TR, double ROW, double s, d3 pts_i, d3 pts_j, d3 vel_i, d3 vel_j, double td_i, double td_j,
                     double uvy_i, double uvy_j, const double *pose_i, const double *pose_j, const double *ex, double lam, double td,
                     double *r, double (*Ji)[6], double (*Jj)[6], double (*Jex)[6], double *Jl, double *Jtd) {
  // tangent base of pts_j (projection_factor.cpp:6-19)
  const double nj0 = sqrt(dot(pts_j, pts_j));
  const d3 a = (1.0 / nj0) * pts_j;
  d3 tmp = mk3(0.0, 0.0, 1.0);
  if (a.x == 0.0 && a.y == 0.0 && a.z == 1.0) tmp = mk3(1.0, 0.0, 0.0);
  d3 b1 = tmp - dot(a, tmp) * a;
  b1 = (1.0 / sqrt(dot(b1, b1))) * b1;
  const d3 b2 = cross(a, b1);
  d3 pi = pts_i, pj = pts_j;
  if (use_td) {
    const double row_i = uvy_i - ROW / 2, row_j = uvy_j - ROW / 2;
    pi = pts_i - (td - td_i + TR / ROW * row_i) * vel_i;
    pj = pts_j - (td - td_j + TR / ROW * row_j) * vel_j;
  }
  const d3 Pi = ld3(pose_i), Pj = ld3(pose_j), tic = ld3(ex);
  const q4 Qi = q_from_pose(pose_i), Qj = q_from_pose(pose_j), qic = q_from_pose(ex);
  const d3 Xci = (1.0 / lam) * pi;
  const d3 Xbi = qrot(qic, Xci) + tic;
  const d3 Xw = qrot(Qi, Xbi) + Pi;
  const d3 Xbj = qrot(qinv(Qj), Xw - Pj);
  const d3 Xcj = qrot(qinv(qic), Xbj - tic);
  const double n = sqrt(dot(Xcj, Xcj)), npj = sqrt(dot(pj, pj));
  const d3 e = (1.0 / n) * Xcj - (1.0 / npj) * pj;
  r[0] = s * dot(b1, e), r[1] = s * dot(b2, e);
  const m33 Ri = q2R(Qi), Rj = q2R(Qj), ric = q2R(qic);
  const m33 RjT = tr(Rj), ricT = tr(ric);
  // red = s B (I / n - X X^T / n^3): 2 x 3
  double red[2][3];
  {
    const double xv[3] = {Xcj.x, Xcj.y, Xcj.z}, bv[2][3] = {{b1.x, b1.y, b1.z}, {b2.x, b2.y, b2.z}};
    const double n3 = n * n * n;
    for (int k = 0; k < 2; k++)
      for (int c = 0; c < 3; c++) {
        double v = 0.0;
        for (int q = 0; q < 3; q++) v += bv[k][q] * ((q == c ? 1.0 / n : 0.0) - xv[q] * xv[c] / n3);
        red[k][c] = s * v;
      }
  }
  auto redm = [&](const m33 &M, double (*out)[6], int c0, double sg) {
    for (int k = 0; k < 2; k++)
      for (int c = 0; c < 3; c++) out[k][c0 + c] = sg * (red[k][0] * M.a[c] + red[k][1] * M.a[3 + c] + red[k][2] * M.a[6 + c]);
  };
  const m33 ricT_RjT = mm(ricT, RjT);
  const m33 M2 = mm(ricT_RjT, Ri);
  m33 nskXbi = skewm(Xbi);
  for (int k = 0; k < 9; k++) nskXbi.a[k] = -nskXbi.a[k];
  redm(ricT_RjT, Ji, 0, 1.0);
  redm(mm(M2, nskXbi), Ji, 3, 1.0);
  redm(ricT_RjT, Jj, 0, -1.0);
  redm(mm(ricT, skewm(Xbj)), Jj, 3, 1.0);
  const m33 T = mm(M2, ric);
  {  // ric^T (Rj^T Ri - I)

    m33 RjRi = mm(RjT, Ri);
    RjRi.a[0] -= 1.0, RjRi.a[4] -= 1.0, RjRi.a[8] -= 1.0;
    redm(mm(ricT, RjRi), Jex, 0, 1.0);
  }
  {
    const d3 cc = mul(ricT, mul(RjT, mul(Ri, tic) + Pi - Pj) - tic);
    m33 B = mm(T, skewm(Xci));
    const m33 S1 = skewm(mul(T, Xci)), S2 = skewm(cc);
    for (int k = 0; k < 9; k++) B.a[k] = -B.a[k] + S1.a[k] + S2.a[k];
    redm(B, Jex, 3, 1.0);
  }
  const d3 Tpi = mul(T, pi), Tvi = mul(T, vel_i);
  for (int k = 0; k < 2; k++) {
    Jl[k] = (red[k][0] * Tpi.x + red[k][1] * Tpi.y + red[k][2] * Tpi.z) * -1.0 / (lam * lam);
    Jtd[k] = (red[k][0] * Tvi.x + red[k][1] * Tvi.y + red[k][2] * Tvi.z) / lam * -1.0 + s * (k == 0 ? vel_j.x : vel_j.y);
  }
}

DEV d3 relo_ld3s(const double *p, int o) { return mk3(p[3 * o], p[3 * o + 1], p[3 * o + 2]); }

// One factor's rows into the row table and the landmark's accumulators.  cols: 19 camera-side columns (pose_i 6 | pose_j 6 |
// ex 6 | td 1), -1 = not a column of the problem.
DEV void relo_put_factor(const ReloDev *D, int row, const double *r, const double (*Jc)[19], const int *cols, const double *Jl, double *w,
                         double &h, double &g) {
  for (int k = 0; k < 2; k++) {
    double *dst = D->J + (size_t)(row + k) * RLD;
    for (int c = 0; c < 19; c++)
      if (cols[c] >= 0) dst[cols[c]] = Jc[k][c];
    dst[RK] = r[k];
    h += Jl[k] * Jl[k];
    g += Jl[k] * r[k];
  }
  for (int c = 0; c < 19; c++)
    if (cols[c] >= 0) w[cols[c]] += Jc[0][c] * Jl[0] + Jc[1][c] * Jl[1];
}

// LIN: rows, w_l, h_l, g_l and cost at x[D->tr.cur]; !LIN: cost only at the candidate x[cur ^ 1].
// Grid: ceil(N / 64) landmark workgroups, then LFVIO_WINDOW_SIZE IMU workgroups, then one prior workgroup; 64 threads.
template <bool LIN>
__global__ void __launch_bounds__(64) k_relo_eval(ReloDev *D) {
  const int tid = threadIdx.x, nlw = (D->N + RELO_LM_WG - 1) / RELO_LM_WG;
  if (D->tr.done || (LIN ? !D->tr.do_lin : D->tr.chol_fail)) return;  // (a pass that keeps its linearization / has no candidate)
  const int cur = LIN ? D->tr.cur : (D->tr.cur ^ 1);
  const ReloX *X = &D->x[cur];
  const double *lam = D->lam[cur];
  const int est_ex = D->est_ex, est_td = D->est_td;
  __shared__ double sh[15 * 31];
  if ((int)blockIdx.x < nlw) {
    const int l = blockIdx.x * RELO_LM_WG + tid;
    if (l >= D->N) return;
    const int o0 = D->off[l], o1 = D->off[l + 1], fi = D->start[l];
    double cost = 0.0, h = 0.0, g = 0.0;
    double *w = LIN ? D->W + (size_t)l * RK : nullptr;
    if (LIN) {  // this lane owns its W row and its factors' rows
      for (int k = 0; k < RK; k++) w[k] = 0.0;
      const int rv = 2 * (o0 - l), nv = 2 * (o1 - o0 - 1);
      for (int e = 0; e < nv * RLD; e++) D->J[(size_t)rv * RLD + e] = 0.0;
      if (D->rk[l] >= 0)
        for (int e = 0; e < 2 * RLD; e++) D->J[(size_t)(D->row_relo + 2 * D->rk[l]) * RLD + e] = 0.0;
    }
    const d3 pi = relo_ld3s(D->pt, o0), vi = relo_ld3s(D->vel, o0);
    const int nf = (o1 - o0 - 1) + (D->rk[l] >= 0 ? 1 : 0);
    for (int q = 0; q < nf; q++) {
      const bool is_relo = q == o1 - o0 - 1;
      double r[2], Ji[2][6], Jj[2][6], Jex[2][6], Jl[2], Jtd[2];
      int fj, row;
      if (!is_relo) {
        const int o = o0 + 1 + q;
        fj = fi + 1 + q;
        row = 2 * (o - l - 1);
        relo_visual(est_td != 0, D->tr_ro, D->row, D->sqrt_info, pi, relo_ld3s(D->pt, o), vi, relo_ld3s(D->vel, o), D->ctd[o0], D->ctd[o],
                    D->uvy[o0], D->uvy[o], X->f.pose[fi], X->f.pose[fj], X->f.ex, lam[l], X->f.td, r, Ji, Jj, Jex, Jl, Jtd);
      } else {
        const int k = D->rk[l];
        fj = -1;
        row = D->row_relo + 2 * k;
        const d3 pj = mk3(D->mp[2 * k], D->mp[2 * k + 1], 1.0), z = mk3(0.0, 0.0, 0.0);
        relo_visual(false, D->tr_ro, D->row, D->sqrt_info, pi, pj, z, z, 0.0, 0.0, 0.0, 0.0, X->f.pose[fi], X->relo, X->f.ex, lam[l], X->f.td, r,
                    Ji, Jj, Jex, Jl, Jtd);
      }
      // ceres::CauchyLoss(1.0) through the Corrector: rho'' = -rho'^2 <= 0, so residual and Jacobian scale by sqrt(rho')
      const double sq_n = r[0] * r[0] + r[1] * r[1];
      cost += 0.5 * log1p(sq_n);
      if (!LIN) continue;
      const double sq = sqrt(1.0 / (1.0 + sq_n));
      double rc[2], Jc[2][19], Jlc[2];
      int cols[19];
      for (int k = 0; k < 2; k++) {
        rc[k] = sq * r[k], Jlc[k] = sq * Jl[k];
        for (int c = 0; c < 6; c++) Jc[k][c] = sq * Ji[k][c], Jc[k][6 + c] = sq * Jj[k][c], Jc[k][12 + c] = sq * Jex[k][c];
        Jc[k][18] = (!is_relo && est_td) ? sq * Jtd[k] : 0.0;
      }
      for (int c = 0; c < 6; c++) {
        cols[c] = off_pose(fi) + c;
        cols[6 + c] = is_relo ? RO + c : off_pose(fj) + c;
        cols[12 + c] = est_ex ? off_ex() + c : -1;
      }
      cols[18] = (!is_relo && est_td) ? off_td() : -1;
      relo_put_factor(D, row, rc, Jc, cols, Jlc, w, h, g);
    }
    D->lcost[l] = cost;
    if (LIN) D->h[l] = h, D->gl[l] = g;
    return;
  }
  const int b = blockIdx.x - nlw;
  if (b < LFVIO_WINDOW_SIZE) {
    // IMUFactor (imu_factor.h:19-200): raw residual and 15 x 30 Jacobian, whitened by sqrt_info (upper triangular)
    const int f = b;
    if (!D->imu_on[f]) {  // (sum_dt > 10 or no LLT: the factor is not in the problem, its rows are zero)
      if (LIN && tid < 15)
        for (int e = 0; e < RLD; e++) D->J[(size_t)(D->row_imu + 15 * f + tid) * RLD + e] = 0.0;
      if (tid == 0) D->pcost[f] = 0.0;
      return;
    }
    double *Jr = sh, *rr = sh + 15 * 30;
    if (tid == 0) {
      for (int k = 0; k < 450; k++) Jr[k] = 0.0;
      imu_raw_residual(&D->imu[f], D->g, X->f.pose[f], X->f.sb[f], X->f.pose[f + 1], X->f.sb[f + 1], rr);
      if (LIN) imu_raw_jacobian(&D->imu[f], D->g, X->f.pose[f], X->f.sb[f], X->f.pose[f + 1], X->f.sb[f + 1], Jr);
    }
    __syncthreads();
    const double *Sq = D->imu_sqrt[f];
    double rw = 0.0;
    if (LIN && tid < 15)
      for (int e = 0; e < RLD; e++) D->J[(size_t)(D->row_imu + 15 * f + tid) * RLD + e] = 0.0;
    if (tid < 15) {
      for (int k = tid; k < 15; k++) rw += Sq[tid * 15 + k] * rr[k];
      if (LIN) {
        double *dst = D->J + (size_t)(D->row_imu + 15 * f + tid) * RLD;
        for (int c = 0; c < 30; c++) {
          double v = 0.0;
          for (int k = tid; k < 15; k++) v += Sq[tid * 15 + k] * Jr[k * 30 + c];
          const int gc = c < 6 ? off_pose(f) + c : c < 15 ? off_sb(f) + (c - 6) : c < 21 ? off_pose(f + 1) + (c - 15) : off_sb(f + 1) + (c - 21);
          dst[gc] = v;
        }
        dst[RK] = rw;
      }
    }
    __syncthreads();
    if (tid < 15) sh[tid] = rw * rw;
    __syncthreads();
    if (tid == 0) {
      double c = 0.0;
      for (int k = 0; k < 15; k++) c += sh[k];
      D->pcost[f] = 0.5 * c;
    }
    return;
  }
  // MarginalizationFactor (marginalization_factor.cpp:329-381): r = r0 + J0 dx
  const int n = D->prior_n;
  if (n == 0) {
    if (tid == 0) D->pcost[LFVIO_WINDOW_SIZE] = 0.0;
    return;
  }
  double *dx = sh;  // n <= 172 < 465
  for (int k = tid; k < n; k += 64) dx[k] = 0.0;
  __syncthreads();
  if (tid == 0)
    for (int bi = 0; bi < D->prior_nb; bi++) prior_block_dx(D->prior_kind[bi], D->prior_frame[bi], D->prior_idx[bi], D->prior_x0[bi], &X->f, dx);
  __syncthreads();
  double c2 = 0.0;
  for (int i = tid; i < n; i += 64) {
    const double *Jrow = D->prior_J + (size_t)i * n;
    double v = D->prior_r[i];
    for (int k = 0; k < n; k++) v += Jrow[k] * dx[k];
    c2 += v * v;
    if (LIN) {
      double *dst = D->J + (size_t)(D->row_prior + i) * RLD;
      for (int e = 0; e < RLD; e++) dst[e] = 0.0;
      for (int bi = 0; bi < D->prior_nb; bi++) {
        const int kind = D->prior_kind[bi], fr = D->prior_frame[bi], idx = D->prior_idx[bi];
        if ((kind == LFVIO_BLOCK_EX_POSE && !est_ex) || (kind == LFVIO_BLOCK_TD && !est_td)) continue;
        const int ls = kind == LFVIO_BLOCK_SPEEDBIAS ? 9 : kind == LFVIO_BLOCK_TD ? 1 : 6;
        const int go = kind == LFVIO_BLOCK_POSE ? off_pose(fr) : kind == LFVIO_BLOCK_SPEEDBIAS ? off_sb(fr) : kind == LFVIO_BLOCK_EX_POSE ? off_ex() : off_td();
        for (int k = 0; k < ls; k++) dst[go + k] += Jrow[idx + k];
      }
      dst[RK] = v;
    }
  }
  __syncthreads();
  double *red = sh + 200;
  red[tid] = c2;
  __syncthreads();
  if (tid == 0) {
    double c = 0.0;
    for (int k = 0; k < 64; k++) c += red[k];
    D->pcost[LFVIO_WINDOW_SIZE] = 0.5 * c;
  }
}

// [H_cc | g_c] partial sums: block (tile, chunk); thread (i, j) of the 16 x 16 tile sums its entry over the chunk's rows.
__global__ void __launch_bounds__(256) k_relo_gram(ReloDev *D) {
  if (D->tr.done || !D->tr.do_lin) return;
  const int t = blockIdx.x, ch = blockIdx.y;
  int a = 0;
  while ((a + 1) * (a + 2) / 2 <= t) a++;
  const int bcol = t - a * (a + 1) / 2;  // tile (a, bcol), bcol <= a
  const int i = a * 16 + (threadIdx.x >> 4), j = bcol * 16 + (threadIdx.x & 15);
  const int R = D->R, per = (R + RELO_GCH - 1) / RELO_GCH, r0 = ch * per, r1 = min(R, r0 + per);
  if (i >= RG || j >= RG) return;
  double s = 0.0;
  const double *J = D->J;
  for (int r = r0; r < r1; r++) s += J[(size_t)r * RLD + i] * J[(size_t)r * RLD + j];
  D->gpart[((size_t)ch * RG + i) * RG + j] = s;
}

DEV int relo_pk(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// the whole augmented state as Ceres' x vector, squared norm of (a) or of (a - b); k_relo_solve's workgroup
DEV double relo_xsq(const ReloDev *D, const ReloX *a, const double *la, const ReloX *b, const double *lb, double *red) {
  const int tid = threadIdx.x;
  double s = 0.0;
  auto acc = [&](double va, double vb) {
    const double d = b ? va - vb : va;
    s += d * d;
  };
  if (tid < LFVIO_NUM_FRAMES) {
    for (int k = 0; k < 7; k++) acc(a->f.pose[tid][k], b ? b->f.pose[tid][k] : 0.0);
    for (int k = 0; k < 9; k++) acc(a->f.sb[tid][k], b ? b->f.sb[tid][k] : 0.0);
  } else if (tid == LFVIO_NUM_FRAMES) {
    if (D->est_ex)
      for (int k = 0; k < 7; k++) acc(a->f.ex[k], b ? b->f.ex[k] : 0.0);
    if (D->est_td) acc(a->f.td, b ? b->f.td : 0.0);
    if (D->relo_on)
      for (int k = 0; k < 7; k++) acc(a->relo[k], b ? b->relo[k] : 0.0);
  }
  for (int l = tid; l < D->N; l += RELO_SOLVE_THREADS) acc(la[l], lb ? lb[l] : 0.0);
  s = block_sum<RELO_SOLVE_THREADS>(s, red, tid);
  __syncthreads();
  return s;
}

// The reduced system of the Gauss-Newton step at the current mu, over 16 x 16 tiles of its lower triangle + the rhs column:
//   S = Hs + mu D_c^2 - sum_l w_l w_l^T / (h_l + mu D_l^2),   rhs = g_c - sum_l w_l g_l / (h_l + mu D_l^2)
// (inactive columns: identity rows, zero rhs).  k_relo_solve factors it; a retry with a raised mu inside k_relo_solve forms
// it there itself.
__global__ void __launch_bounds__(256) k_relo_schur(ReloDev *D) {
  const TRState *T = &D->tr;
  if (T->done || !T->do_schur) return;
  const int t = blockIdx.x;
  int i, j;
  if (t == RELO_GTILES) {  // the last workgroup: the rhs column
    i = threadIdx.x, j = RK;
    if (i >= RK) return;
  } else {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= t) a++;
    const int bcol = t - a * (a + 1) / 2;
    i = a * 16 + (threadIdx.x >> 4), j = bcol * 16 + (threadIdx.x & 15);
    if (i >= RK || j > i) return;
  }
  const double mu = T->mu;
  const int N = D->N;
  const double *W = D->W, *hs = D->hs, *dl = D->diag_l, *gsl = D->gsl;
  double v;
  if (j == RK) {
    v = D->gs[i];
    if (D->act[i])
      for (int l = 0; l < N; l++) v -= W[(size_t)l * RK + i] * gsl[l] / (hs[l] + mu * dl[l] * dl[l]);
    if (!D->act[i]) v = 0.0;
  } else if (!D->act[i] || !D->act[j]) {
    v = i == j ? 1.0 : 0.0;
  } else {
    v = D->Hs[i * RK + j] + (i == j ? mu * D->diag[i] * D->diag[i] : 0.0);
    for (int l = 0; l < N; l++) v -= W[(size_t)l * RK + i] * W[(size_t)l * RK + j] / (hs[l] + mu * dl[l] * dl[l]);
  }
  D->Sg[(size_t)i * (RK + 1) + j] = v;
  if (t == 0 && threadIdx.x == 0) D->Sg_mu = mu;
}

// One pass of the loop up to the candidate.  D->tr.do_lin: a new linearization lies in the row table / W / h / g (its
// gradient closes the last trace entry); D->tr.do_schur: the Gauss-Newton step has to be (re)computed with the current mu.
__global__ void __launch_bounds__(RELO_SOLVE_THREADS) k_relo_solve(ReloDev *D, int phase) {
  extern __shared__ double lds[];
  double *A = lds, *rhs = lds + RPACK, *hinv = rhs + RK, *red = hinv + RELO_MAX_LM;
  const int tid = threadIdx.x, nt = blockDim.x, N = D->N;
  TRState *T = &D->tr;
  if (T->done) return;
  const int cur = T->cur;
  if (phase == 0) {
    if (!T->do_lin) return;
    const bool first = !T->scaled;  // the start point: IterationZero
    // H_cc | g_c from the chunk partials (fixed order), unscaled
    for (int e = tid; e < RK * RK; e += nt) {
      const int i = e / RK, j = e % RK, a = max(i, j), b = min(i, j);
      double s = 0.0;
      for (int c = 0; c < RELO_GCH; c++) s += D->gpart[((size_t)c * RG + a) * RG + b];
      D->Hs[e] = s;
    }
    __syncthreads();
    // gradient of the new point (unscaled J^T r): Ceres' gradient_max_norm = max |x - Plus(x, -g)|
    double gm = 0.0;
    const ReloX *X = &D->x[cur];
    auto gcol = [&](int i) {
      double s = 0.0;
      for (int c = 0; c < RELO_GCH; c++) s += D->gpart[((size_t)c * RG + RK) * RG + i];
      return s;
    };
    if (tid < RK) D->gs[tid] = gcol(tid);
    __syncthreads();
    auto pose_gm = [&](const double *xb, int o) {
      double d[6], xo[7], m = 0.0;
      for (int k = 0; k < 6; k++) d[k] = -D->gs[o + k];
      pose_plus(xb, d, xo);
      for (int k = 0; k < 7; k++) m = fmax(m, fabs(xb[k] - xo[k]));
      return m;
    };
    if (tid < LFVIO_NUM_FRAMES) gm = pose_gm(X->f.pose[tid], off_pose(tid));
    else if (tid == LFVIO_NUM_FRAMES && D->est_ex) gm = pose_gm(X->f.ex, off_ex());
    else if (tid == LFVIO_NUM_FRAMES + 1 && D->relo_on) gm = pose_gm(X->relo, RO);
    else if (tid == LFVIO_NUM_FRAMES + 2 && D->est_td) gm = fabs(D->gs[off_td()]);
    if (tid < 99) gm = fmax(gm, fabs(D->gs[off_sb(0) + tid]));
    for (int l = tid; l < N; l += nt) gm = fmax(gm, fabs(D->gl[l]));
    gm = block_max<RELO_SOLVE_THREADS>(gm, red, tid);
    __syncthreads();
    // Jacobi scaling, fixed at the start point (trust_region_minimizer.cc: jacobian_scaling = 1 / (1 + |J_col|))
    if (first) {
      if (tid < RK) D->scale[tid] = D->act[tid] ? 1.0 / (1.0 + sqrt(D->Hs[tid * RK + tid])) : 1.0;
      for (int l = tid; l < N; l += nt) D->scale_l[l] = 1.0 / (1.0 + sqrt(D->h[l]));
      __syncthreads();
    }
    // scaled system, D diagonal (dogleg_strategy.cc: sqrt of the clamped column norms of the scaled Jacobian)
    for (int e = tid; e < RK * RK; e += nt) {
      const int i = e / RK, j = e % RK;
      D->Hs[e] = (D->act[i] && D->act[j]) ? D->Hs[e] * D->scale[i] * D->scale[j] : 0.0;
    }
    if (tid < RK) {
      D->gs[tid] = D->act[tid] ? D->gs[tid] * D->scale[tid] : 0.0;
    }
    for (int e = tid; e < N * RK; e += nt) {
      const int l = e / RK, i = e % RK;
      D->W[e] = D->act[i] ? D->W[e] * D->scale[i] * D->scale_l[l] : 0.0;
    }
    for (int l = tid; l < N; l += nt) {
      const double sl = D->scale_l[l];
      D->hs[l] = D->h[l] * sl * sl;
      D->gsl[l] = D->gl[l] * sl;
      D->diag_l[l] = sqrt(fmin(fmax(D->hs[l], 1e-6), 1e32));
    }
    __syncthreads();
    if (tid < RK) D->diag[tid] = D->act[tid] ? sqrt(fmin(fmax(D->Hs[tid * RK + tid], 1e-6), 1e32)) : 1.0;
    __syncthreads();
    // Cauchy point: alpha = |grad|^2 / |J (grad / D)|^2, grad = g / D
    double g2 = 0.0, q = 0.0;
    if (tid < RK && D->act[tid]) {
      const double v = D->gs[tid] / (D->diag[tid] * D->diag[tid]);
      double hv = 0.0;
      for (int k = 0; k < RK; k++) hv += D->Hs[tid * RK + k] * (D->act[k] ? D->gs[k] / (D->diag[k] * D->diag[k]) : 0.0);
      q += v * hv;
      g2 += (D->gs[tid] / D->diag[tid]) * (D->gs[tid] / D->diag[tid]);
    }
    for (int l = tid; l < N; l += nt) {
      const double dl = D->diag_l[l], vl = D->gsl[l] / (dl * dl);
      double wv = 0.0;
      const double *w = D->W + (size_t)l * RK;
      for (int k = 0; k < RK; k++) wv += w[k] * (D->act[k] ? D->gs[k] / (D->diag[k] * D->diag[k]) : 0.0);
      q += 2.0 * vl * wv + D->hs[l] * vl * vl;
      g2 += (D->gsl[l] / dl) * (D->gsl[l] / dl);
    }
    double gq[2] = {g2, q};
    block_sum_n<RELO_SOLVE_THREADS>(gq, red, tid);
    __syncthreads();
    if (tid == 0) {
      T->alpha = gq[0] / gq[1];
      if (first) {
        double c = 0.0;
        for (int l = 0; l < N; l++) c += D->lcost[l];
        for (int k = 0; k < RELO_PCOST; k++) c += D->pcost[k];
        T->x_cost = c, T->initial_cost = c;
        LfvioIterationSummary it;
        it.cost = c, it.cost_change = 0, it.gradient_max_norm = gm, it.step_norm = 0, it.relative_decrease = 0;
        it.trust_region_radius = T->radius, it.step_is_valid = 0, it.step_is_successful = 0;
        T->trace[0] = it;
        T->trace_len = 1;
      } else if (T->trace_len > 0 && T->trace_len <= LFVIO_MAX_TRACE) {
        T->trace[T->trace_len - 1].gradient_max_norm = gm;
      }
      if (gm <= 1e-10) T->termination = LFVIO_CONVERGENCE, T->done = 1;  // GradientToleranceReached
      if (first && !T->done && T->iteration >= D->max_iter) T->termination = LFVIO_NO_CONVERGENCE, T->done = 1;
    }
    if (first) {
      const double xn = relo_xsq(D, &D->x[cur], D->lam[cur], nullptr, nullptr, red);
      if (tid == 0) T->x_norm = sqrt(xn);
    }
    __syncthreads();
    if (tid == 0) {
      T->do_lin = 0;
      if (first) T->scaled = 1, T->iteration = 1;  // (the candidate of the next pass is Ceres' iteration 1: decide_walk counts from there)
    }
    __syncthreads();
    return;
  }
  if (T->do_schur) {
    // Gauss-Newton step of (J^T J + mu D^T D) y = J^T r through the Schur complement of the (diagonal) landmark block;
    // a failed factorization raises mu (LinearSolver failure -> mu *= 10 while mu < 1: dogleg_strategy.cc ComputeGaussNewtonStep)
    bool ok = false;
    double mu = T->mu;
    while (mu < 1.0) {
      for (int l = tid; l < N; l += nt) hinv[l] = 1.0 / (D->hs[l] + mu * D->diag_l[l] * D->diag_l[l]);
      __syncthreads();
      const bool pre = mu == D->Sg_mu;  // (k_relo_schur formed the system at this mu)
      for (int e = tid; e < RPACK + RK; e += nt) {
        int i, j;
        if (e < RPACK) {
          i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
          while (i * (i + 1) / 2 > e) i--;
          while ((i + 1) * (i + 2) / 2 <= e) i++;
          j = e - i * (i + 1) / 2;
        } else {
          i = e - RPACK, j = -1;
        }
        double v;
        if (pre) {
          if (j >= 0) A[e] = D->Sg[(size_t)i * (RK + 1) + j];
          else rhs[i] = D->Sg[(size_t)i * (RK + 1) + RK];
          continue;
        }
        if (j >= 0) {
          if (!D->act[i] || !D->act[j]) {
            v = i == j ? 1.0 : 0.0;
          } else {
            v = D->Hs[i * RK + j] + (i == j ? mu * D->diag[i] * D->diag[i] : 0.0);
            for (int l = 0; l < N; l++) {
              const double *w = D->W + (size_t)l * RK;
              v -= w[i] * w[j] * hinv[l];
            }
          }
          A[e] = v;
        } else {
          v = D->gs[i];
          if (D->act[i])
            for (int l = 0; l < N; l++) v -= D->W[(size_t)l * RK + i] * D->gsl[l] * hinv[l];
          rhs[i] = D->act[i] ? v : 0.0;
        }
      }
      __syncthreads();
      // packed right-looking Cholesky
      __shared__ int fail;
      if (tid == 0) fail = 0;
      __syncthreads();
      for (int k = 0; k < RK; k++) {
        const double dkk = A[relo_pk(k, k)];
        if (!(dkk > 0.0) || !isfinite(dkk)) {
          if (tid == 0) fail = 1;
          break;
        }
        const double d = sqrt(dkk);
        __syncthreads();
        if (tid == 0) A[relo_pk(k, k)] = d;
        for (int i = k + 1 + tid; i < RK; i += nt) A[relo_pk(i, k)] /= d;
        __syncthreads();
        const int m = RK - 1 - k;
        for (int e = tid; e < m * m; e += nt) {
          const int i = k + 1 + e / m, j = k + 1 + e % m;
          if (j <= i) A[relo_pk(i, j)] -= A[relo_pk(i, k)] * A[relo_pk(j, k)];
        }
        __syncthreads();
      }
      __syncthreads();
      if (!fail) {
        // L y = rhs, L^T x = y
        for (int k = 0; k < RK; k++) {
          const double yk = rhs[k] / A[relo_pk(k, k)];
          __syncthreads();
          if (tid == 0) rhs[k] = yk;
          for (int i = k + 1 + tid; i < RK; i += nt) rhs[i] -= A[relo_pk(i, k)] * yk;
          __syncthreads();
        }
        for (int k = RK - 1; k >= 0; k--) {
          const double xk = rhs[k] / A[relo_pk(k, k)];
          __syncthreads();
          if (tid == 0) rhs[k] = xk;
          for (int i = tid; i < k; i += nt) rhs[i] -= A[relo_pk(k, i)] * xk;
          __syncthreads();
        }
        int bad = 0;
        if (tid < RK) {
          const double y = D->act[tid] ? rhs[tid] : 0.0;
          if (!isfinite(y)) bad = 1;
          D->gn[tid] = -D->diag[tid] * y;
        }
        for (int l = tid; l < N; l += nt) {
          const double *w = D->W + (size_t)l * RK;
          double v = D->gsl[l];
          for (int k = 0; k < RK; k++) v -= w[k] * (D->act[k] ? rhs[k] : 0.0);
          const double y = v * hinv[l];
          if (!isfinite(y)) bad = 1;
          D->gn_l[l] = -D->diag_l[l] * y;
        }
        const double nb = block_max<RELO_SOLVE_THREADS>((double)bad, red, tid);
        __syncthreads();
        if (nb == 0.0) {
          ok = true;
          break;
        }
      }
      __syncthreads();
      mu *= 10.0;
    }
    __syncthreads();
    if (tid == 0) {
      T->mu = mu;
      T->chol_fail = ok ? 0 : 1;
      T->do_schur = 0;
    }
    __syncthreads();
  }
  if (T->chol_fail) return;
  // dogleg (dogleg_strategy.cc ComputeTraditionalDoglegStep): step = cg grad + cn gn in the D-scaled space
  double dn[3] = {0.0, 0.0, 0.0};  // |g / D|^2, |gn|^2, (g / D).gn
  if (tid < RK && D->act[tid]) {
    const double gr = D->gs[tid] / D->diag[tid];
    dn[0] += gr * gr, dn[1] += D->gn[tid] * D->gn[tid], dn[2] += gr * D->gn[tid];
  }
  for (int l = tid; l < N; l += nt) {
    const double gr = D->gsl[l] / D->diag_l[l];
    dn[0] += gr * gr, dn[1] += D->gn_l[l] * D->gn_l[l], dn[2] += gr * D->gn_l[l];
  }
  block_sum_n<RELO_SOLVE_THREADS>(dn, red, tid);
  __syncthreads();
  const double gg = dn[0], nn = dn[1], gnv = dn[2];
  const double radius = T->radius, alpha = T->alpha, gnorm = sqrt(gg), gnn = sqrt(nn);
  double cg, cn, dsn;
  if (gnn <= radius) {
    cg = 0.0, cn = 1.0, dsn = gnn;
  } else if (gnorm * alpha >= radius) {
    cg = -(radius / gnorm), cn = 0.0, dsn = radius;
  } else {
    const double b_dot_a = -alpha * gnv, a2 = (alpha * gnorm) * (alpha * gnorm);
    const double bma2 = a2 - 2.0 * b_dot_a + gnn * gnn, c = b_dot_a - a2;
    const double d = sqrt(c * c + bma2 * (radius * radius - a2));
    const double beta = c <= 0 ? (d - c) / bma2 : (radius * radius - a2) / (d + c);
    cg = -alpha * (1.0 - beta), cn = beta;
    dsn = sqrt(cg * cg * gg + 2.0 * cg * cn * gnv + cn * cn * nn);
  }
  // s = step / D; model_cost_change = -s.g - s^T H s / 2
  if (tid < RK) D->stp[tid] = D->act[tid] ? (cg * D->gs[tid] / D->diag[tid] + cn * D->gn[tid]) / D->diag[tid] : 0.0;
  for (int l = tid; l < N; l += nt) D->stp_l[l] = (cg * D->gsl[l] / D->diag_l[l] + cn * D->gn_l[l]) / D->diag_l[l];
  __syncthreads();
  double mq[2] = {0.0, 0.0};  // s.g, s^T H s
  if (tid < RK && D->act[tid]) {
    double hv = 0.0;
    for (int k = 0; k < RK; k++) hv += D->Hs[tid * RK + k] * D->stp[k];
    mq[0] += D->stp[tid] * D->gs[tid], mq[1] += D->stp[tid] * hv;
  }
  for (int l = tid; l < N; l += nt) {
    const double *w = D->W + (size_t)l * RK;
    double wv = 0.0;
    for (int k = 0; k < RK; k++) wv += w[k] * D->stp[k];
    const double sl = D->stp_l[l];
    mq[0] += sl * D->gsl[l], mq[1] += 2.0 * sl * wv + D->hs[l] * sl * sl;
  }
  block_sum_n<RELO_SOLVE_THREADS>(mq, red, tid);
  __syncthreads();
  // candidate x (+) (s * scale)
  const ReloX *X = &D->x[cur];
  ReloX *Y = &D->x[cur ^ 1];
  if (tid < LFVIO_NUM_FRAMES) {
    double d[6];
    for (int k = 0; k < 6; k++) d[k] = D->stp[off_pose(tid) + k] * D->scale[off_pose(tid) + k];
    pose_plus(X->f.pose[tid], d, Y->f.pose[tid]);
    for (int k = 0; k < 9; k++) Y->f.sb[tid][k] = X->f.sb[tid][k] + D->stp[off_sb(tid) + k] * D->scale[off_sb(tid) + k];
  } else if (tid == LFVIO_NUM_FRAMES) {
    if (D->est_ex) {
      double d[6];
      for (int k = 0; k < 6; k++) d[k] = D->stp[off_ex() + k] * D->scale[off_ex() + k];
      pose_plus(X->f.ex, d, Y->f.ex);
    } else {
      for (int k = 0; k < 7; k++) Y->f.ex[k] = X->f.ex[k];
    }
    Y->f.td = D->est_td ? X->f.td + D->stp[off_td()] * D->scale[off_td()] : X->f.td;
  } else if (tid == LFVIO_NUM_FRAMES + 1) {
    if (D->relo_on) {
      double d[6];
      for (int k = 0; k < 6; k++) d[k] = D->stp[RO + k] * D->scale[RO + k];
      pose_plus(X->relo, d, Y->relo);
    } else {
      for (int k = 0; k < 7; k++) Y->relo[k] = X->relo[k];
    }
  }
  for (int l = tid; l < N; l += nt) D->lam[cur ^ 1][l] = D->lam[cur][l] + D->stp_l[l] * D->scale_l[l];
  __syncthreads();
  const double sn2 = relo_xsq(D, Y, D->lam[cur ^ 1], X, D->lam[cur], red);
  const double xn2 = relo_xsq(D, Y, D->lam[cur ^ 1], nullptr, nullptr, red);
  if (tid == 0) {
    D->mlin = mq[0], D->mquad = mq[1];
    T->dogleg_step_norm = dsn;
    T->step_sq_pose = sn2;
    T->xn2_pose_cand = xn2;
  }
}

// TrustRegionMinimizer's bookkeeping for the candidate of the pass: decide_walk on one lane, as k_decide's decide_body does, with
// one candidate whose whole model terms, step and state norms are in mlin / mquad, step_sq_pose and xn2_pose_cand.  (Its retry
// branch, chol_fail with mu < 1, is not met here: k_relo_solve raises mu to 1 before it reports a failed factorization.)
__global__ void k_relo_decide(ReloDev *D) {
  if (threadIdx.x != 0 || D->tr.done) return;
  DecideSums sm = {};
  for (int l = 0; l < D->N; l++) sm.cost[0] += D->lcost[l];
  for (int k = 0; k < RELO_PCOST; k++) sm.cost[0] += D->pcost[k];
  sm.mlin[0] = D->mlin, sm.mquad[0] = D->mquad;
  TRHead t = *reinterpret_cast<const TRHead *>(&D->tr);
  decide_walk(t, sm, 1, 0, D->max_iter, &D->tr);
  TRDecision d;
  decision_from(d, t, 0);
  decision_to_header(&D->tr, d);
}

// IMU sqrt_info = LLT(covariance^-1).matrixL()^T (imu_factor.h:37-38): Gauss-Jordan inverse with partial pivoting, then the
// column Cholesky; one lane per interval.  State and header of the loop.
__global__ void __launch_bounds__(64) k_relo_setup(ReloDev *D, double init_radius, double fn_tol) {
  __shared__ double M[LFVIO_WINDOW_SIZE][15][30];
  const int f = threadIdx.x;
  if (f < LFVIO_WINDOW_SIZE) {
    double(*m)[30] = M[f];
    const double *P = D->imu[f].covariance;
    for (int i = 0; i < 15; i++)
      for (int j = 0; j < 30; j++) m[i][j] = j < 15 ? P[i * 15 + j] : (j - 15 == i ? 1.0 : 0.0);
    bool ok = !(D->imu[f].sum_dt > 10.0);  // estimator.cpp:720
    for (int k = 0; k < 15 && ok; k++) {
      int p = k;
      for (int i = k + 1; i < 15; i++)
        if (fabs(m[i][k]) > fabs(m[p][k])) p = i;
      if (m[p][k] == 0.0) {
        ok = false;
        break;
      }
      if (p != k)
        for (int j = 0; j < 30; j++) {
          const double t = m[k][j];
          m[k][j] = m[p][j], m[p][j] = t;
        }
      const double piv = m[k][k];
      for (int j = 0; j < 30; j++) m[k][j] /= piv;
      for (int i = 0; i < 15; i++)
        if (i != k) {
          const double fct = m[i][k];
          if (fct != 0.0)
            for (int j = 0; j < 30; j++) m[i][j] -= fct * m[k][j];
        }
    }
    // Cholesky of the inverse (columns 15..29), lower L in place of columns 0..14
    double L[15][15];
    for (int i = 0; i < 15; i++)
      for (int j = 0; j < 15; j++) L[i][j] = 0.0;
    for (int j = 0; j < 15 && ok; j++) {
      double t = m[j][15 + j];
      for (int k = 0; k < j; k++) t -= L[j][k] * L[j][k];
      if (!(t > 0.0)) {
        ok = false;
        break;
      }
      L[j][j] = sqrt(t);
      for (int i = j + 1; i < 15; i++) {
        double v = m[i][15 + j];
        for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
        L[i][j] = v / L[j][j];
      }
    }
    for (int i = 0; i < 15; i++)
      for (int j = 0; j < 15; j++) D->imu_sqrt[f][i * 15 + j] = (ok && j >= i) ? L[j][i] : 0.0;
    D->imu_on[f] = ok ? 1 : 0;
  }
  for (int l = threadIdx.x; l < D->N; l += blockDim.x) D->lam[0][l] = D->lam0[l], D->lam[1][l] = D->lam0[l];
  if (threadIdx.x == 0) {
    D->x[0] = D->x0;
    D->x[1] = D->x0;
    tr_init(&D->tr, init_radius, fn_tol);  // (the host zeroed the rest of the header)
  }
}

// "Maximum solver time reached": the loop ends where it is, termination NO_CONVERGENCE
__global__ void k_relo_stop(ReloDev *D) {
  if (threadIdx.x == 0 && !D->tr.done) D->tr.done = 1, D->tr.termination = LFVIO_NO_CONVERGENCE;
}
